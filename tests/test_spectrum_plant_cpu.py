"""The planted spectrum inputs of tests/spectrum_plant.py, checked without a GPU: every case has the per-part counts it claims.

tests/test_gpu_spectrum_planted.py runs the same cases through the kernels; what makes them bite — a counter at exactly 15 in a
given part, one at 16, a run across a part border — is a property of the input and of the mirror of the launch rule, and is pinned
here: the oracle's histograms equal the planned totals, the mirror's per-part counts equal the planned per-part counts, the cases
that must not overflow keep every (part, bin) counter at or below 15 and the ones that must have exactly the intended counters at
16 or above."""
import os
import re

import numpy as np
import pytest

import spectrum_plant as sp
from conftest import pack_reads
from oracle import pyorc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hulk_amd", "csrc")
ALL = sp.all_cases()
IDS = [f"{leg}-{name}" for leg, name in ALL]

# (leg-independent) the counters each case means to take to 16 or beyond: {case name: number of such (part, bin) counters}
OVERFLOWS = {"threshold_16_n7": 1, "threshold_16_n3": 1, "threshold_17_31": 2, "flag_middle_4096": 1, "flag_middle_4100": 1,
             "border_k23_16": 2, "border_k31_16": 2}


_ORACLES = {}


def _oracle(k):
    """one oracle per k for all cases (its tables take half a second to draw), wiped between spectra; no interval: never flushed"""
    if k not in _ORACLES:
        _ORACLES[k] = pyorc.Sketcher(k, 1, 1, 0, 1.0, 0)
    return _ORACLES[k]


def test_the_mirror_follows_the_sources():
    """the constants and the rules that spectrum_plant.Launch / launches() copy are the ones the library is built with"""
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("hulk_spectrum.hip", "hulk_flush.hip", "hulk_api.hip", "hulk_internal.h")}
    s = src["hulk_spectrum.hip"]
    post = s[s.index("hipError_t launch_minimizer_post("):]
    assert "constexpr int FAST_READS_PER_WAVE = 16;" in src["hulk_internal.h"] and sp.REGION == 16
    assert "constexpr int SCAN_BATCH_MAX = 16;" in src["hulk_internal.h"] and sp.BATCH_DEFAULT == 16
    assert "c->ring_n = c->T + 1;" in src["hulk_api.hip"]
    assert "ml.nib_parts = 48;" in src["hulk_flush.hip"] and sp.NIB_PARTS == 48
    assert "ml.max_parts = 8;" in src["hulk_flush.hip"] and sp.EXACT_MAX_PARTS == 8
    # the 4-bit launch: 131072 keys per part and 2^18-bin range, 128 workgroups from 4096 reads up, at most 48 parts and 8192 workgroups
    assert "#define HULK_NIB_RLOG_DEFAULT 18" in s and "#define HULK_NIB_BLOCK_DEFAULT 1024" in s
    assert "constexpr int NIB_BINS_MAX = 262144;" in s
    assert "const uint64_t rps = P.interval ? std::min<uint64_t>(P.interval, n_reads) : n_reads;" in post
    assert "keys_env > 0 ? (uint64_t)keys_env : 131072ull * (uint64_t)nr18;" in post and sp.NIB_KEYS == 131072
    assert "uint32_t np = (uint32_t)((rps * 20 + keys_per_part - 1) / keys_per_part);" in post
    assert 'min_blocks = em ? atoi(em) : 128;' in post and sp.NIB_MIN_BLOCKS == 128
    assert ("if (rps >= 4096 && (uint64_t)np * n_spectra * nr < (uint64_t)min_blocks) np = (uint32_t)(((uint64_t)min_blocks + "
            "(uint64_t)n_spectra * nr - 1) / ((uint64_t)n_spectra * nr));") in post and sp.NIB_MIN_READS == 4096
    assert "if (np > ml.nib_parts) np = ml.nib_parts;" in post
    assert "while (np > 1 && (uint64_t)np * n_spectra * nr > 8192) np--;" in post and sp.NIB_MAX_BLOCKS == 8192
    assert "return v < 13 ? 13 : v > 18 ? 18 : v;" in post and "return v == 256 || v == 512 ? v : 1024;" in post
    # the exact launch: ranges of 2^15 bins, 512 workgroups, at most 8 parts, one part below 65536 reads
    assert "constexpr int HIST_RANGE = 32768;" in s and 1 << sp.EXACT_RANGE_LOG == 32768
    assert "parts_target = ep ? atoi(ep) : 512;" in post and sp.EXACT_BLOCKS == 512
    assert "uint32_t n_parts = (uint32_t)parts_target / (uint32_t)(nranges * n_spectra);" in post
    assert "if (n_reads < 65536) n_parts = 1;" in post and sp.EXACT_MIN_READS == 65536
    assert "n_spectra = P.interval ? (uint32_t)((P.fill + n_reads + P.interval - 1) / P.interval) : 1u;" in post
    # a part of a spectrum's key list, in both histogram kernels
    part = ("const uint32_t g0 = (uint32_t)(rd0 / FAST_READS_PER_WAVE), g1 = (uint32_t)((rd1 - 1) / FAST_READS_PER_WAVE);\n"
            "        const uint32_t a = ml.off[g0], b = ml.off[(g1 + 1 < n_regions ? g1 + 1 : n_regions)];\n"
            "        const uint32_t len = b - a, per = (len + n_parts - 1) / n_parts;\n"
            "        const uint32_t lo = a + (uint32_t)part * per, hi = (lo + per < b) ? lo + per : b;")
    assert s.count(part) == 2
    assert s.count("const uint32_t slot = P.interval ? (uint32_t)(((uint64_t)t + P.ring_base) % P.ring_n) : P.ring_base;") >= 4
    # the interval rule of the host calls
    a = src["hulk_api.hip"]
    assert "const uint64_t fill = I ? c->seq_count % I : 0;" in a
    assert "if (I) { const uint64_t room = (uint64_t)c->T * I - fill; if (chunk > room) chunk = room; }" in a
    assert re.search(r"c->ring_base = \(c->ring_base \+ done\) % c->ring_n;\s+if \(\(fill \+ chunk\) % I == 0\) \{ c->ring_base = 0;", a)


def test_the_geometries_the_cases_are_meant_to_have():
    g = {(leg, name): sp.case(leg, name).launches[-1].geometry() for leg, name in ALL}
    assert g[("default", "threshold_15")] == [1, 1, 1, 18, 1024]
    assert g[("default", "merge")] == [1, 48, 1, 18, 1024]
    assert sp.case("default", "merge").launches[0].keys_of(0) == (0, 4608, 96)          # 48 parts of 6 regions
    assert g[("default", "parts43")] == g[("default", "flag_middle_4096")] == g[("default", "flag_middle_4100")] == [3, 43, 1, 18, 1024]
    assert g[("default", "ring_slots")] == [3, 1, 1, 18, 1024]
    assert g[("default", "border_k23_15")] == [1, 48, 2, 18, 1024] and g[("default", "border_k31_16")] == [1, 32, 4, 18, 1024]
    assert g[("default", "parts_beyond_end")] == [2, 48, 1, 18, 1024]
    assert [sp.case("default", f"head_tail_{n}").launches[0].keys_of(0)[2] % 4 for n in (4609, 4700, 4750)] == [1, 2, 3]
    assert g[("rlog13", "merge")] == [1, 6, 24, 13, 256] and g[("rlog16", "merge")] == [1, 43, 3, 16, 256]
    assert g[("exact", "exact_merge")] == [1, 8, 6, 15, 1024]
    assert [sp.case("exact", f"head_tail_{n}").launches[0].keys_of(0)[2] % 4 for n in (65537, 65546, 65555)] == [1, 2, 3]
    assert all(sp.case("exact", n).launches[0].np == 8 for n in sp.EXACT_CASES)


@pytest.mark.parametrize("leg,name", ALL, ids=IDS)
def test_oracle_histograms_equal_the_planned_totals(leg, name):
    """every interval of the stream through the oracle on its own: the histogram is the planned one, bin for bin, and every read
    has exactly one minimizer"""
    c = sp.case(leg, name)
    assert all(len(r) == c.k for r in c.reads) and not any(b"N" in r for r in c.reads[:64])
    totals = c.spectrum_totals()
    step = c.interval or c.n
    o = _oracle(c.k)
    for s, want in totals.items():
        o.wipe()
        before = o.counters()["n_minimizers"]
        o.add_reads(*pack_reads(c.reads[s * step:(s + 1) * step]))
        got = o.histogram()
        n_min = o.counters()["n_minimizers"] - before
        assert n_min == min(step, c.n - s * step) == int(want.sum())
        assert np.array_equal(got.astype(np.uint32), want), f"interval {s}: {int((got != want).sum())} bins differ"
        if c.finish:
            assert np.count_nonzero(want) >= 0.01 * c.k ** 4, "the spectrum would fail the reference's 1 % rule"


@pytest.mark.parametrize("leg,name", ALL, ids=IDS)
def test_per_part_counts_equal_the_plan(leg, name):
    """the mirror's count of every planted (launch, spectrum, part, bin) is the planned one; nothing else is above 1; a region cut
    by a part border holds fillers only (head_tail / parts_beyond_end: planted runs cross the borders on purpose, and a run is
    all of its bin: 15 keys)"""
    c = sp.case(leg, name)
    counts = c.part_counts()
    planted = {}
    for (l, t, p), d in c.plants.items():
        for b, v in d.items():
            planted[(l, t, p, b)] = v
            assert counts[(l, t, p)][b] == v, (l, t, p, b)
    for (l, t, p), ctr in counts.items():
        for b, v in ctr.items():
            if v > 1 and (l, t, p, b) not in planted:
                assert b in c.loose and v <= c.loose[b] == 15, (l, t, p, b, v)
    totals = c.spectrum_totals()
    for b, v in c.loose.items():
        assert sum(int(h[b]) for h in totals.values()) == v == 15
    if not c.loose:
        for L in c.launches:
            for t in range(L.n_spectra):
                cut = [L.first + i for i in L.cut_region_reads(t)]
                assert not set(int(x) for x in c.bins[cut]) & c.planted_bins, "a planted copy sits in a region that a part border cuts"
    # parts of one spectrum cover its keys exactly once
    for li, L in enumerate(c.launches):
        for t in range(L.n_spectra):
            assert sum(sum(counts[(li, t, p)].values()) for p in range(L.np)) == max(L.reads_of(t)[1] - L.reads_of(t)[0], 0)


@pytest.mark.parametrize("leg,name", ALL, ids=IDS)
def test_counters_reach_16_exactly_where_intended(leg, name):
    c = sp.case(leg, name)
    over = c.overflows()
    if name not in OVERFLOWS:
        top = max(max(ctr.values(), default=0) for ctr in c.part_counts().values())
        assert not over and top <= 15 and (top == 15 or c.loose)      # (a run that crosses part borders is 15 keys in all)
        assert c.flags() == [0] * c.launches[-1].n_spectra
        return
    want = {(l, t, p, b) for (l, t, p), d in c.plants.items() for b, v in d.items() if v >= 16}
    assert over == want and len(over) == OVERFLOWS[name]
    flagged = sorted({t for (l, t, p, b) in over})
    assert c.flags() == [1 if t in flagged else 0 for t in range(c.launches[-1].n_spectra)]
    if name.startswith("flag_middle"):
        assert c.flags() == [0, 1, 0]


def test_the_search_fails_loudly_at_its_cap():
    with pytest.raises(RuntimeError, match="cap"):
        bk = sp.ReadBank(31, seed=5, cap=sp.ReadBank.CHUNK)
        for b in range(31 ** 4 - 64, 31 ** 4):
            bk.read(b)


def test_the_search_agrees_with_the_oracle_on_random_reads():
    """the numpy transcription that finds the reads and the oracle that accepts them, on k-mers of every k the cases use"""
    for k in (21, 23, 31):
        bk = sp.bank(k)
        bins = np.nonzero(bk.have)[0][:: max(bk.have.sum() // 300, 1)]
        for b in bins:
            assert bk.bin_of(bk.read(b)) == b
