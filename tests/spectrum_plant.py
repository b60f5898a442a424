"""Planted inputs for the 4-bit k-mer spectrum (k_nibble_hist -> k_nibble_merge -> k_recount_flagged in hulk_spectrum.hip) and
for the exact 32-bit path (k_range_hist -> k_merge_hist).

The spectrum kernels count the dense key list of a launch in parts: a launch rule cuts every spectrum's keys into `np` parts, one
workgroup counts one (part, bin range) in LDS — with four-bit counters, eight bins to a word — and a merge sums the parts.  What
can go wrong there depends on WHICH counter of WHICH part holds what, so the inputs here are built backwards from per-(part, bin)
counts:

  * a read of exactly k bases has one k-mer, so at w = 1 it yields one key; its bin is jump(value, k^4).  ReadBank draws random
    k-mers from a seed and keeps one read per bin; a read for any wanted bin, or for any bin of a wanted word, is then at hand.
    The search for a bin runs on a numpy transcription of the hash and of the jump hash; every read that is handed out is then put
    through the CPU oracle (exactly one minimizer, and the bin the search promised).
  * launches() / Launch restate hulk_add_reads_device's interval rule and launch_minimizer_post's part rule (the constants are
    checked against the sources by tests/test_spectrum_plant_cpu.py, the numbers against the library's own through the hook
    HULK_DEBUG_NIBBLE by tests/test_gpu_spectrum_planted.py).  The key list is dense in read order, one region per 16 reads; with
    one key per read the key index is the read index up to the order inside a region.
  * Case.plant() takes per-(launch, spectrum, part, bin) counts and places the copies in whole regions that lie inside that part; every
    other read, those of a region cut by a part border among them, is a filler read with a bin of its own (count 1), so the order
    inside a region never matters.  Enough fillers make a spectrum pass the reference's 1 % rule where a case goes on to finish().

No read has an N or is of low complexity beyond what a random k-mer is: such reads would be deferred to the generic kernel and
never enter the key list.
"""
import collections

import numpy as np

from oracle import pyorc

REGION = 16                     # reads per region of the key list (FAST_READS_PER_WAVE)
NIB_PARTS = 48                  # parts the lane's 4-bit buffer holds (ml.nib_parts)
NIB_KEYS = 131072               # keys per part and range of 2^18 bins
NIB_MIN_READS, NIB_MIN_BLOCKS, NIB_MAX_BLOCKS = 4096, 128, 8192
EXACT_RANGE_LOG, EXACT_BLOCKS, EXACT_MAX_PARTS, EXACT_MIN_READS = 15, 512, 8, 65536
BATCH_DEFAULT = 16
U64 = np.uint64


# ------------------------------------------------------------------------------------------------- reads with one key
def _hash64(key, mask):
    """minimap2's invertible hash, as oracle/hulk_oracle.c has it, on uint64 arrays"""
    key = (~key + (key << U64(21))) & mask
    key = key ^ (key >> U64(24))
    key = ((key + (key << U64(3))) + (key << U64(8))) & mask
    key = key ^ (key >> U64(14))
    key = ((key + (key << U64(2))) + (key << U64(4))) & mask
    key = key ^ (key >> U64(28))
    key = (key + (key << U64(31))) & mask
    return key


def _jump(keys, n):
    """go-jump on a uint64 array (the same doubles as the reference: one division, one product, truncation)"""
    keys = keys.copy()
    out = np.zeros(len(keys), dtype=np.int64)
    live = np.arange(len(keys))
    b = np.zeros(len(keys), dtype=np.int64)
    while len(live):
        keys = keys * U64(2862933555777941757) + U64(1)
        j = ((b + 1).astype(np.float64) * (2147483648.0 / ((keys >> U64(33)) + U64(1)).astype(np.float64))).astype(np.int64)
        done = j >= n
        out[live[done]] = b[done]
        keep = ~done
        live, keys, b = live[keep], keys[keep], j[keep]
    return out


class ReadBank:
    """One verified k-base read per bin of the k^4-bin spectrum, found from a seed.  `cap` bounds the k-mers drawn: a search that
    reaches it fails loudly."""
    CHUNK = 1 << 19

    def __init__(self, k, seed, cap=1 << 25):
        self.k, self.B, self.cap = k, k ** 4, cap
        self._rng = np.random.default_rng(seed)
        self.drawn = 0
        self._code = np.zeros(self.B, dtype=np.uint64)          # forward k-mer (2 bits per base) of the read kept for a bin
        self.have = np.zeros(self.B, dtype=bool)
        self._verified = {}                                       # bin -> read, through the oracle
        self._grow()

    def _grow(self):
        if self.drawn + self.CHUNK > self.cap:
            raise RuntimeError(f"ReadBank(k={self.k}): {self.drawn} k-mers drawn, the cap of {self.cap} is reached")
        k = self.k
        fwd = self._rng.integers(0, 1 << (2 * k), size=self.CHUNK, dtype=np.uint64)
        rc = np.zeros_like(fwd)
        x = fwd.copy()
        for _ in range(k):                                        # reverse complement: 3 ^ base, last base first
            rc = (rc << U64(2)) | (U64(3) ^ (x & U64(3)))
            x >>= U64(2)
        ok = fwd != rc                                            # a self-complementary k-mer (even k) yields no minimizer
        mask = U64((1 << (2 * k)) - 1)
        value = (_hash64(np.minimum(fwd, rc), mask) << U64(8)) | U64(k)
        bins = _jump(value, self.B)
        new = ok & ~self.have[bins]
        idx = np.nonzero(new)[0][::-1]                            # (reversed: of several reads of a bin the first drawn stays)
        self._code[bins[idx]] = fwd[idx]
        self.have[bins[idx]] = True
        self.drawn += self.CHUNK

    def read(self, b):
        """the read whose one key falls into bin b"""
        b = int(b)
        if b not in self._verified:
            assert 0 <= b < self.B
            while not self.have[b]:
                self._grow()
            code = int(self._code[b])
            seq = bytes(b"ACGT"[(code >> (2 * (self.k - 1 - i))) & 3] for i in range(self.k))
            m = pyorc.minimizers(seq, self.k, 1)
            if len(m) != 1 or pyorc.jump(int(m[0]), self.B) != b:
                raise RuntimeError(f"ReadBank(k={self.k}): the oracle puts {seq!r} into {[pyorc.jump(int(v), self.B) for v in m]}, not into bin {b}")
            self._verified[b] = seq
        return self._verified[b]

    def bin_of(self, seq):
        m = pyorc.minimizers(seq, self.k, 1)
        assert len(m) == 1
        return pyorc.jump(int(m[0]), self.B)

    def word_with(self, nibbles, after=1, avoid=()):
        """first word (8 bins) from word `after` on whose bins at `nibbles` all have a read and that is none of `avoid`"""
        full = self.B // 8
        ok = np.ones(full, dtype=bool)
        for nb in nibbles:
            ok &= self.have[nb:full * 8:8]
        ok[:after] = False
        for w in avoid:
            if w < full:
                ok[w] = False
        w = np.nonzero(ok)[0]
        if not len(w):
            raise RuntimeError(f"ReadBank(k={self.k}): no word holds reads for nibbles {nibbles}")
        return int(w[0])

    def border(self, log2_range, avoid_words=()):
        """(m * 2^log2_range - 1, m * 2^log2_range): two bins either side of a range border, both with a read"""
        step = 1 << log2_range
        for edge in range(step, self.B, step):
            if self.have[edge - 1] and self.have[edge] and (edge - 1) // 8 not in avoid_words and edge // 8 not in avoid_words:
                return edge - 1, edge
        raise RuntimeError(f"ReadBank(k={self.k}): no border of 2^{log2_range}-bin ranges has reads on both sides")

    def fillers(self, n, exclude):
        """n bins that have a read, in ascending order, none of them in `exclude`"""
        while True:
            ok = self.have.copy()
            ok[list(exclude)] = False
            bins = np.nonzero(ok)[0]
            if len(bins) >= n:
                # spread over the whole bin range, so that every range and most words see a filler
                return bins[(np.arange(n) * len(bins)) // n]
            self._grow()


_BANKS = {}


def bank(k):
    if k not in _BANKS:
        _BANKS[k] = ReadBank(k, seed=1000 + k)
    return _BANKS[k]


# ------------------------------------------------------------------------------------------------- the launch rule
def ceil_div(a, b):
    return -(-a // b)


class Launch:
    """One binning launch: reads [first, first + n) of the stream, `fill` reads already in its first spectrum, which lies on ring
    slot `ring_base`.  Mirrors launch_minimizer_post (hulk_spectrum.hip): the geometry of the 4-bit kernels (rlog / block: the
    profiling build's HULK_NIB_RLOG / HULK_NIB_BLOCK) or, exact=True (HULK_NO_NIBBLE), of k_range_hist / k_merge_hist."""

    def __init__(self, k, first, n, interval, fill, ring_base, ring_n, rlog=18, block=1024, exact=False):
        self.k, self.B, self.first, self.n, self.interval, self.fill = k, k ** 4, first, n, interval, fill
        self.ring_base, self.ring_n = ring_base, ring_n
        self.n_spectra = ceil_div(fill + n, interval) if interval else 1
        self.n_regions = ceil_div(n, REGION)
        if exact:
            self.nr, self.rlog, self.block = ceil_div(self.B, 1 << EXACT_RANGE_LOG), EXACT_RANGE_LOG, 1024
            np_ = max(EXACT_BLOCKS // (self.nr * self.n_spectra), 1)
            np_ = min(np_, EXACT_MAX_PARTS)
            if n < EXACT_MIN_READS:
                np_ = 1
        else:
            self.nr, self.rlog, self.block = ceil_div(self.B, 1 << rlog), rlog, block
            nr18 = ceil_div(self.B, 1 << 18)
            rps = min(interval, n) if interval else n
            np_ = max(ceil_div(rps * 20, NIB_KEYS * nr18), 1)
            if rps >= NIB_MIN_READS and np_ * self.n_spectra * self.nr < NIB_MIN_BLOCKS:
                np_ = ceil_div(NIB_MIN_BLOCKS, self.n_spectra * self.nr)
            np_ = min(np_, NIB_PARTS)
            while np_ > 1 and np_ * self.n_spectra * self.nr > NIB_MAX_BLOCKS:
                np_ -= 1
        self.np = np_

    def geometry(self):
        """what HULK_DEBUG_NIBBLE reports: spectra, parts, ranges, log2 of a range's bins, workgroup threads"""
        return [self.n_spectra, self.np, self.nr, self.rlog, self.block]

    def slot(self, t):
        return (t + self.ring_base) % self.ring_n if self.interval else self.ring_base

    def reads_of(self, t):
        """[rd0, rd1): the launch's reads (local index) that belong to spectrum t"""
        if not self.interval:
            return 0, self.n
        lo, hi = t * self.interval, (t + 1) * self.interval
        return max(lo - self.fill, 0), min(max(hi - self.fill, 0), self.n)

    def spectrum_of(self, rd):
        return (self.fill + rd) // self.interval if self.interval else 0

    def keys_of(self, t):
        """(a, b, per): the key range of spectrum t (whole regions around its reads) and the length of a part"""
        rd0, rd1 = self.reads_of(t)
        if rd0 >= rd1:
            return 0, 0, 0
        g0, g1 = rd0 // REGION, (rd1 - 1) // REGION
        a, b = g0 * REGION, min((g1 + 1) * REGION, self.n)        # one key per read: off[g] = 16 g, off[n_regions] = n
        return a, b, ceil_div(b - a, self.np)

    def part(self, t, p):
        """[lo, hi) of part p of spectrum t in the launch's key list; hi < lo for a part beyond the end of a short list"""
        a, b, per = self.keys_of(t)
        lo = a + p * per
        return lo, (lo + per if lo + per < b else b)

    def whole_region_reads(self, t, p):
        """local indices of the reads of spectrum t in regions that lie wholly inside part p and inside the spectrum"""
        lo, hi = self.part(t, p)
        rd0, rd1 = self.reads_of(t)
        lo, hi = max(lo, rd0), min(hi, rd1)
        g0, g1 = ceil_div(lo, REGION), hi // REGION
        return list(range(g0 * REGION, g1 * REGION)) if g1 > g0 else []

    def cut_region_reads(self, t):
        """local indices of all reads in regions that a part border of spectrum t runs through"""
        out = set()
        a, b, per = self.keys_of(t)
        for p in range(1, self.np):
            lo = a + p * per
            if lo < b and lo % REGION:
                g = lo // REGION
                out.update(range(g * REGION, min((g + 1) * REGION, self.n)))
        return out


def launches(k, calls, interval=0, batch=0, **kw):
    """hulk_add_reads_device's loop: the launches that host calls of `calls` reads each turn into"""
    T = batch or BATCH_DEFAULT
    ring_n = T + 1
    seq, ring_base, out = 0, 0, []
    for n in calls:
        pos = 0
        while pos < n:
            fill = seq % interval if interval else 0
            chunk = n - pos
            if interval:
                chunk = min(chunk, T * interval - fill)
            out.append(Launch(k, seq, chunk, interval, fill, ring_base, ring_n, **kw))
            seq += chunk
            pos += chunk
            if interval:
                done = (fill + chunk) // interval
                ring_base = (ring_base + done) % ring_n
                if (fill + chunk) % interval == 0:
                    ring_base = 0
    return out


# ------------------------------------------------------------------------------------------------- cases
class Case:
    """A planted input: `reads` for the host calls `calls`, the plan it was built from (`plants`: {(launch, spectrum, part):
    {bin: count}}, `loose`: {bin: count} of copies placed by read index, see head_tail()) and what the launch must report."""

    def __init__(self, name, k, calls, interval=0, batch=0, work_lanes=0, finish=False, rlog=18, block=1024, exact=False):
        self.name, self.k, self.calls, self.interval, self.batch, self.work_lanes, self.finish = name, k, list(calls), interval, batch, work_lanes, finish
        self.exact = exact
        self.launches = launches(k, calls, interval, batch, rlog=rlog, block=block, exact=exact)
        self.n = sum(calls)
        self.bins = np.full(self.n, -1, dtype=np.int64)         # bin of every read's key
        self.plants = collections.OrderedDict()
        self.loose = {}
        self.reads = None

    # ---- building
    def plant(self, launch, t, part, counts):
        """counts: {bin: copies} for part `part` of spectrum t of launch `launch` — into whole regions inside that part"""
        L = self.launches[launch]
        key = (launch, t, part)
        self.plants.setdefault(key, {})
        free = [L.first + i for i in L.whole_region_reads(t, part) if self.bins[L.first + i] < 0]
        need = sum(counts.values())
        assert need <= len(free), f"{self.name}: part {key} has {len(free)} free reads in whole regions, {need} wanted"
        at = 0
        for b, c in counts.items():
            self.plants[key][b] = self.plants[key].get(b, 0) + c
            self.bins[free[at:at + c]] = b
            at += c

    def plant_at(self, first, b, count):
        """`count` copies of bin b at reads first, first + 1, ... wherever the part borders are (head_tail())"""
        assert (self.bins[first:first + count] < 0).all()
        self.bins[first:first + count] = b
        self.loose[b] = self.loose.get(b, 0) + count

    def close(self, distinct_over_case=False):
        """every read that holds no planted copy gets a filler bin of its own (distinct within its spectrum; the same filler bins
        serve every spectrum).  Returns self."""
        bk = bank(self.k)
        planted = set(int(b) for b in self.bins[self.bins >= 0])
        spectrum = np.zeros(self.n, dtype=np.int64)              # stream-wide interval number of every read
        if self.interval:
            spectrum = np.arange(self.n) // self.interval
        per_spec = collections.Counter(spectrum[self.bins < 0].tolist())
        fill_bins = bk.fillers(max(per_spec.values(), default=0), planted)
        for s, cnt in per_spec.items():
            idx = np.nonzero((self.bins < 0) & (spectrum == s))[0]
            self.bins[idx] = fill_bins[:cnt]
        self.reads = [bk.read(b) for b in self.bins]
        self.planted_bins = planted
        return self

    # ---- what the plan implies
    def spectrum_totals(self):
        """{stream-wide interval number: histogram} as planned (uint32[k^4] each)"""
        out = {}
        spec = np.arange(self.n) // self.interval if self.interval else np.zeros(self.n, dtype=np.int64)
        for s in np.unique(spec):
            out[int(s)] = np.bincount(self.bins[spec == s], minlength=self.k ** 4).astype(np.uint32)
        return out

    def part_counts(self):
        """{(launch, spectrum, part): Counter(bin -> keys)} by the mirror, keys in read order"""
        out = {}
        for li, L in enumerate(self.launches):
            local = self.bins[L.first:L.first + L.n]
            spec = np.array([L.spectrum_of(i) for i in range(L.n)]) if L.interval else np.zeros(L.n, dtype=np.int64)
            for t in range(L.n_spectra):
                for p in range(L.np):
                    lo, hi = L.part(t, p)
                    if hi <= lo:
                        out[(li, t, p)] = collections.Counter()
                        continue
                    seg = local[lo:hi][spec[lo:hi] == t]
                    out[(li, t, p)] = collections.Counter(seg.tolist())
        return out

    def overflows(self):
        """{(launch, spectrum, part, bin)} whose counter reaches 16 or more"""
        return {(l, t, p, b) for (l, t, p), c in self.part_counts().items() for b, v in c.items() if v >= 16}

    def flags(self):
        """nib_over[0 .. n_spectra) as the LAST launch must leave it (all 0 on the exact path, which has no 4-bit counters)"""
        last = len(self.launches) - 1
        f = [0] * self.launches[last].n_spectra
        if not self.exact:
            for (l, t, p, b) in self.overflows():
                if l == last:
                    f[t] = 1
        return f


def _threshold_layout(bk, rlog):
    """bins of the one-part threshold cases: bin 0 (nibble 0 of the first word), the lone last bin, a word W with reads for
    nibbles 0, 3, 4, 6, 7 and a word V for nibbles 0 and 7; at rlog < 18 two bins either side of a range border"""
    W = bk.word_with((0, 3, 4, 6, 7))
    V = bk.word_with((0, 7), avoid=(W,))
    lay = dict(first=0, last=bk.B - 1, W=W, V=V)
    if rlog < 18:
        lay["border"] = bk.border(rlog, avoid_words=(0, W, V))
    return lay


def threshold(variant, rlog=18, block=1024, k=21, n=1600):
    """One part (fewer than 4,096 reads), one spectrum.  variant "15": counters at 1, 14 and 15 — at nibble 0 and nibble 7 of a
    word, in bin 0 and in the lone last bin; a 15 whose same-word neighbours also hold 15.  No counter reaches 16.
    "16_n7": the same with nibble 7 of W at 16 (the carry leaves the word); "16_n3": nibble 3 at 16 (the carry runs into nibble
    4, which holds 15); "17_31": nibble 3 at 17 and nibble 7 at 31."""
    bk = bank(k)
    lay = _threshold_layout(bk, rlog)
    W, V = lay["W"] * 8, lay["V"] * 8
    counts = {lay["first"]: 15, lay["last"]: 15, W + 0: 14, W + 3: 15, W + 4: 15, W + 6: 15, W + 7: 15, V + 0: 15, V + 7: 1}
    if "border" in lay:
        counts[lay["border"][0]] = 15
        counts[lay["border"][1]] = 15
    if variant == "16_n7":
        counts[W + 7] = 16
    elif variant == "16_n3":
        counts[W + 3] = 16
    elif variant == "17_31":
        counts[W + 3], counts[W + 7] = 17, 31
    else:
        assert variant == "15"
    c = Case(f"threshold_{variant}", k, [n], rlog=rlog, block=block)
    c.plant(0, 0, 0, counts)
    return c.close()


def merge(rlog=18, block=1024, k=21, n=4608, exact=False, borders=()):
    """Every part holds 15 of three adjacent bins b, b + 1, b + 2 of one word (both the even and the odd byte lane of the merge
    reach 120 in every step of eight parts); one bin is at 15 in part 0 only and one in the last part only; `borders`: pairs of
    bins either side of a range border, at 15 each in part 1 (or in the only part).
    What this does and does not see of the byte lanes: 8 x 15 = 120 is the most a four-bit part can add per step, and it shows
    a wrong mask, a lane swap or a lost carry between lanes.  A step widened to 16 parts (240) or 17 (255) would still fit a byte;
    only from 18 parts per step on would these counts overflow a lane, so a modest widening is not caught here by overflow."""
    bk = bank(k)
    c = Case("merge", k, [n], rlog=rlog, block=block, exact=exact)
    L = c.launches[0]
    W = bk.word_with((2, 3, 4))
    X = bk.word_with((1, 6), avoid=(W,))
    b = W * 8 + 2
    pairs = list(borders)
    if not exact and rlog < 18:
        pairs.append(bk.border(rlog, avoid_words=(W, X)))
    for p in range(L.np):
        c.plant(0, 0, p, {b: 15, b + 1: 15, b + 2: 15})
    c.plant(0, 0, 0, {X * 8 + 1: 15})
    c.plant(0, 0, L.np - 1, {X * 8 + 6: 15})
    for lo, hi in pairs:
        c.plant(0, 0, min(1, L.np - 1), {lo: 15, hi: 15})
    return c.close()


def three_spectra(variant, interval=4096, k=21):
    """Three spectra in one launch, 43 parts each (no multiple of 8).  "parts43": 15s in the last part (42) and in part 40, where
    the `p + x < n_parts` guard of the eight-wide merge step decides; a first host call of six spectra on the same work lane
    leaves non-zero counters in the lane's part buffer where parts 43..47 of the three-spectra launch would lie (6 spectra x 22
    parts reach the words of (part 43, spectrum 0..2)), so a merge that reads past its last part sees them.
    "flag_middle": the outer spectra hold bins at exactly 15, the middle one a 16 in one part: flags [0, 1, 0].
    An interval that is no multiple of 16 makes regions straddle spectra."""
    bk = bank(k)
    W = bk.word_with((0, 1, 7))
    if variant == "parts43":
        c = Case("parts43", k, [6 * interval, 3 * interval], interval=interval, work_lanes=1, finish=True)
        L = c.launches[1]
        assert c.launches[0].np * 6 > 43 * 3 + 2
        for t in range(3):
            c.plant(1, t, L.np - 1, {W * 8 + 0: 15, W * 8 + 1: 15})
            c.plant(1, t, 40, {W * 8 + 0: 15, W * 8 + 7: 15})
            c.plant(1, t, 0, {W * 8 + 1: 15})
        return c.close()
    assert variant == "flag_middle"
    c = Case(f"flag_middle_{interval}", k, [3 * interval], interval=interval, finish=True)
    L = c.launches[0]
    c.plant(0, 0, 5, {W * 8 + 0: 15, W * 8 + 1: 15})
    c.plant(0, 1, 7, {W * 8 + 0: 15, W * 8 + 1: 16})
    c.plant(0, 1, L.np - 1, {W * 8 + 7: 15})
    c.plant(0, 2, 9, {W * 8 + 0: 15, W * 8 + 1: 15})
    return c.close()


def ring_slots(k=21, interval=2048):
    """batch = 3 (a ring of 4 spectra), host calls of 2.5 intervals: five spectra on slots 0, 1, 2, 3, 0 — the ring wraps.  Every
    spectrum holds 15 in a bin of the last full word and in the lone last bin.  hist + b0 is 16-byte aligned on slots that are a
    multiple of 4 only (k^4 is odd), so slot 0 takes the uint4 write path of the merge and slots 1, 2, 3 the scalar one."""
    c = Case("ring_slots", k, [interval * 5 // 2, interval * 5 // 2], interval=interval, batch=3, finish=True)
    B = k ** 4
    assert B % 8 == 1
    counts = {B - 2: 15, B - 1: 15}                               # nibble 7 of the last full word, and the lone last bin
    slots = []
    for li, L in enumerate(c.launches):
        assert L.np == 1
        for t in range(L.n_spectra):
            if li == 1 and t == 0:
                continue                                         # the second half of interval 2: planted in launch 0
            c.plant(li, t, 0, counts)
            slots.append(L.slot(t))
    assert slots == [0, 1, 2, 3, 0], slots
    return c.close()


def range_border(k, at16):
    """k = 23 (two ranges of 2^18 bins, 48 parts): bins 262,143 and 262,144 and the last bin 279,840; k = 31 (four ranges, 32
    parts): the bins either side of 786,432 and the last bin 923,520 — at 15 (no flag) or, at16, one of each pair at 16 (flag)."""
    bk = bank(k)
    edge = {23: 262144, 31: 786432}[k]
    n = {23: 4608, 31: 4096}[k]
    c = Case(f"border_k{k}_{16 if at16 else 15}", k, [n])
    L = c.launches[0]
    assert L.np == {23: 48, 31: 32}[k]
    c.plant(0, 0, 0, {edge - 1: 15, edge: 15})
    c.plant(0, 0, L.np - 1, {edge - 1: 15, edge: 16 if at16 else 15, k ** 4 - 1: 15})
    c.plant(0, 0, 3, {k ** 4 - 1: 16 if at16 else 15, edge - 1: 15})
    return c.close()


def parts_beyond_end(k=21, interval=4096, extra=100):
    """Two spectra; the second is `extra` reads long, so with 48 parts a part is 3 keys and the last parts start at or after the
    end of its key list.  histogram() is that second spectrum, and it is all this case checks: a spectrum of 100 keys cannot pass
    the reference's 1 % rule, so the case cannot go on to finish() and cms(); the first spectrum therefore holds fillers only
    (nothing planted that no assertion would see) and is there to make the launch one of 4,096 reads per spectrum."""
    c = Case("parts_beyond_end", k, [interval + extra], interval=interval)
    L = c.launches[0]
    a, b, per = L.keys_of(1)
    assert L.np == 48 and a + (L.np - 1) * per >= b, (L.np, a, b, per)
    bk = bank(k)
    W = bk.word_with((0, 7))
    c.plant_at(interval + 2, W * 8 + 0, 15)                      # (a run of 15 spans five parts of 3 keys)
    c.plant_at(interval + extra - 16, W * 8 + 7, 15)
    return c.close()


def head_tail(n, k=21, exact=False):
    """per = ceil(n / parts) is 1, 2 or 3 mod 4, so parts start off a multiple of 4 keys and the kernels' head (up to the 16-byte
    aligned body) and tail (behind it) are up to 3 keys each.  A run of 15 copies of a bin of its own starts at the first read of
    every part and another ends at its last: the keys around every part border are planted copies whatever the order inside a
    region, and no bin has more than 15 keys in all, so no counter can reach 16."""
    c = Case(f"head_tail_{n}", k, [n], exact=exact)
    L = c.launches[0]
    a, b, per = L.keys_of(0)
    assert per % 4 and per >= 32 and a + (L.np - 1) * per + 30 <= b
    bk = bank(k)
    bins = bk.fillers(2 * L.np + 7, ())[5:]                      # any bins with a read, all different
    for p in range(L.np):
        lo, hi = L.part(0, p)
        c.plant_at(lo, int(bins[2 * p]), 15)
        c.plant_at(hi - 15, int(bins[2 * p + 1]), 15)
    return c.close()


def exact_merge(k=21, n=65536):
    """the merge plan on the exact 32-bit path (8 parts from 65,536 reads up), with bins either side of 32,768 and of 163,840"""
    c = merge(k=k, n=n, exact=True, borders=((32767, 32768), (163839, 163840)))
    c.name = "exact_merge"
    return c


# ------------------------------------------------------------------------------------------------- the legs
# name -> builder(rlog=, block=) of the cases that run at the default launch shape (both libraries)
DEFAULT_CASES = collections.OrderedDict([
    ("threshold_15", lambda **kw: threshold("15", **kw)),
    ("threshold_16_n7", lambda **kw: threshold("16_n7", **kw)),
    ("threshold_16_n3", lambda **kw: threshold("16_n3", **kw)),
    ("threshold_17_31", lambda **kw: threshold("17_31", **kw)),
    ("merge", lambda **kw: merge(**kw)),
    ("parts43", lambda **kw: three_spectra("parts43")),
    ("flag_middle_4096", lambda **kw: three_spectra("flag_middle", 4096)),
    ("flag_middle_4100", lambda **kw: three_spectra("flag_middle", 4100)),
    ("ring_slots", lambda **kw: ring_slots()),
    ("border_k23_15", lambda **kw: range_border(23, False)),
    ("border_k23_16", lambda **kw: range_border(23, True)),
    ("border_k31_15", lambda **kw: range_border(31, False)),
    ("border_k31_16", lambda **kw: range_border(31, True)),
    ("parts_beyond_end", lambda **kw: parts_beyond_end()),
    ("head_tail_4609", lambda **kw: head_tail(4609)),
    ("head_tail_4700", lambda **kw: head_tail(4700)),
    ("head_tail_4750", lambda **kw: head_tail(4750)),
])
_SHAPED = ["threshold_15", "threshold_16_n7", "threshold_16_n3", "threshold_17_31", "merge"]
EXACT_CASES = collections.OrderedDict([
    ("exact_merge", lambda: exact_merge()),
    ("head_tail_65537", lambda: head_tail(65537, exact=True)),
    ("head_tail_65546", lambda: head_tail(65546, exact=True)),
    ("head_tail_65555", lambda: head_tail(65555, exact=True)),
])
# leg -> (environment of the profiling build, case names)
LEGS = collections.OrderedDict([
    ("default", ({}, list(DEFAULT_CASES))),
    ("rlog13", ({"HULK_NIB_RLOG": "13", "HULK_NIB_BLOCK": "256"}, _SHAPED)),       # 24 ranges at k = 21
    ("rlog16", ({"HULK_NIB_RLOG": "16", "HULK_NIB_BLOCK": "256"}, _SHAPED)),       # 3 ranges
    ("exact", ({"HULK_NO_NIBBLE": "1"}, list(EXACT_CASES))),                       # k_range_hist / k_merge_hist
])
_BUILT = {}


def case(leg, name):
    """the case `name` as leg `leg` runs it (built once)"""
    if (leg, name) not in _BUILT:
        if leg == "exact":
            c = EXACT_CASES[name]()
        else:
            env = LEGS[leg][0]
            c = DEFAULT_CASES[name](rlog=int(env.get("HULK_NIB_RLOG", 18)), block=int(env.get("HULK_NIB_BLOCK", 1024)))
        _BUILT[(leg, name)] = c
    return _BUILT[(leg, name)]


def all_cases():
    return [(leg, name) for leg, (env, names) in LEGS.items() for name in names]
