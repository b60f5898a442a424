#!/usr/bin/env python3
"""Randomised differential test: libhulkhip (GPU) vs the CPU oracle over random parameters and inputs.
usage: fuzz_parity.py [n_cases] [seed]     (run on the GPU box; prints every mismatch and a summary)
FUZZ_SNAPSHOTS=1: the GPU context records a sketch snapshot after every flushed spectrum (GpuSketcher(snapshots=1)) and every
one of them is compared with the oracle fed the same reads one interval at a time; the draws of a seed do not change."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401  (before libhulkhip, see hulk_amd/_lib.py)
import hulk_amd
from hulk_amd._lib import HulkError
from oracle import pyorc
from conftest import pack_reads

only = int(os.environ["FUZZ_ONLY"]) if "FUZZ_ONLY" in os.environ else None      # run just this case (the others only draw their random numbers)
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = np.random.default_rng(seed)
ALPH = [b"ACGT", b"ACGT", b"ACGTN", b"ACGTacgt", b"ACGTNnRYU\x00\x03", b"AC"]
bad = 0
n_err = 0
errs = {}
t_start = time.time()
budget = float(os.environ.get("FUZZ_SECONDS", 0))                    # stop after this many seconds (the summary counts the cases done)
for case in range(n_cases):
    if budget and time.time() - t_start > budget:
        n_cases = case
        break
    k = int(rng.choice([3, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, 21, 21, 21] + ([27, 28, 31] if os.environ.get("FUZZ_BIG_K") else [])))   # k^4 bins and S*k^4 tables stay small; 21 = the compiled-in default
    w = int(rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 10, 11, 12, 13, 14, 15, 16, 17, 25, 40] if os.environ.get("FUZZ_WIDE_W") else [1, 2, 3, 4, 5, 9, 9, 9, 10, 16, 17, 25, 40]))   # (FUZZ_WIDE_W: every window size of the short-read kernel; changes what a seed draws)
    S = int(rng.choice([1, 2, 7, 8, 9, 16, 31, 50]))
    if k == 21:
        S = min(S, 16)
    if k > 21:
        S = min(S, 2)                  # (FUZZ_BIG_K) 923,521 bins at k = 31: tables of 3 x S x k^4 doubles on both sides
    decay = float(rng.choice([1.0, 1.0, 1.0, 0.0, 0.02, 0.3, 0.97]))
    interval = int(rng.choice([0, 0, 1, 7, 50, 333]))
    batch = int(rng.choice([1, 2, 5, 8, 16]))
    lanes = int(rng.choice([1, 2, 2]))                         # work lanes: batches on alternating streams
    alph = ALPH[int(rng.integers(0, len(ALPH)))]
    n = int(rng.integers(1, 1500))
    lo = w + k - 1
    shape = int(rng.integers(0, 5))
    if shape == 0:
        lens = rng.integers(lo, lo + 40, size=n)
    elif shape == 1:
        lens = rng.integers(lo, 300, size=n) if lo < 300 else np.full(n, lo)
    elif shape == 2:
        lens = np.full(n, max(lo, 150))
    elif shape == 3:
        lens = rng.integers(lo, 3000, size=max(1, n // 10))
    else:
        lens = np.concatenate([rng.integers(lo, lo + 200, size=max(1, n // 2)), rng.integers(1100, 9000, size=3)])
    if not os.environ.get("FUZZ_LEGACY_GEN"):
        # The 1 % rule (kmerspectrum.go:84-96) needs k^4 / 100 used bins per flush: as drawn, a third of the cases ended in "not
        # used yet" on both sides (profiles/r05_soak_9900.txt: 1,271 of 3,929) and compared nothing else.  Scale the reads with k:
        # an interval gets the reads whose minimizers fill > 1 % of the bins (2.5x margin), the stream a whole number of them —
        # or a ragged tail that is long enough itself; 4 % of the cases stay as drawn, so the error path keeps its coverage.
        # (FUZZ_LEGACY_GEN=1: the generator of rounds 1-5; a seed draws other cases now.)
        need = int(np.ceil(0.01 * k ** 4))
        per_read = max(1.0, 2.0 * (float(np.mean(lens)) - k + 1) / (w + 1))      # distinct minimizers of a random read, roughly
        if len(alph) == 2:
            per_read = min(per_read, 8.0)                                     # (two-letter reads repeat their k-mers)
        if rng.random() >= 0.04:
            want = int(np.ceil(2.5 * need / per_read))
            if interval and interval < want:
                interval = want
            total = max(len(lens), want)
            if interval:
                total = ((total + interval - 1) // interval) * interval
                if interval > want and rng.random() < 0.3:
                    total += int(rng.integers(want, interval))                  # a ragged last interval that still passes the rule
            lens = np.tile(lens, -(-total // len(lens)))[:total]
    a = np.frombuffer(alph, dtype=np.uint8)
    seqs = []
    for L in lens:
        s = a[rng.integers(0, len(a), size=int(L))]
        if rng.random() < 0.1 and L > 60:                       # internal repeat / low complexity
            s[20:40] = s[0:20]
        if rng.random() < 0.05:
            s[:] = s[0]
        seqs.append(bytes(s))
    desc = f"case {case}: k={k} w={w} S={S} decay={decay} I={interval} batch={batch} lanes={lanes} alph={alph!r} reads={len(seqs)} shape={shape}"
    oerr = gerr = None
    if os.environ.get("FUZZ_DUMP") == str(case):           # write the case's reads (no GPU needed) and stop
        np.save(os.environ.get("FUZZ_DUMP_FILE", "fuzz_case.npy"), np.array(seqs, dtype=object), allow_pickle=True)
        print("dumped", desc)
        sys.exit(0)
    if (only is not None and case != only) or case < int(os.environ.get("FUZZ_FROM", "0")):
        rng.integers(0, len(seqs) + 1, size=3)
        continue
    o = pyorc.Sketcher(k, w, S, 0, decay, interval)
    bases, offsets = pack_reads(seqs)
    ohist = ghist = None
    try:
        o.add_reads(bases, offsets)
        if interval == 0:
            ohist = o.histogram().astype(np.uint32)          # the whole k-mer spectrum, before the final flush wipes it
        o.finish()
    except pyorc.OracleError as e:
        oerr = str(e)
    if os.environ.get("FUZZ_ORACLE_ONLY"):                    # (no GPU: how many cases of this generator end in an error — CPU-side check)
        if oerr is not None:
            n_err += 1; errs[oerr] = errs.get(oerr, 0) + 1
        rng.integers(0, len(seqs) + 1, size=3)
        o.close()
        continue
    snap = bool(os.environ.get("FUZZ_SNAPSHOTS"))
    n_spectra = (len(seqs) + interval - 1) // interval if interval else 1
    g = hulk_amd.GpuSketcher(k, w, S, interval, decay, batch=batch, work_lanes=lanes,
                             **(dict(snapshots=1, snapshot_capacity=n_spectra + 1) if snap else {}))
    try:
        cuts = sorted(set([0, len(seqs)] + [int(x) for x in rng.integers(0, len(seqs) + 1, size=3)]))
        for x, y in zip(cuts[:-1], cuts[1:]):
            g.add_reads(bases, offsets[x:y + 1])
        if interval == 0:
            ghist = g.histogram()
        g.finish()
    except HulkError as e:
        gerr = e.message
    ok = True
    if ohist is not None and ghist is not None and not np.array_equal(ohist, ghist):
        ok = False; why = f"spectra differ in {int((ohist != ghist).sum())} bins"
    elif (oerr is None) != (gerr is None) or (oerr is not None and oerr != gerr):
        ok = False; why = f"errors differ: oracle={oerr!r} gpu={gerr!r}"
    elif oerr is None:
        om, ow = o.sketch(); gm, gw = g.sketch()
        if not np.array_equal(om, gm):
            ok = False; why = f"{int((om != gm).sum())} of {S} mins differ"
        elif not np.allclose(gw, ow, rtol=1e-7 if decay != 1.0 else 1e-9, atol=0):
            ok = False; why = "weights differ: max rel %.3g" % float(np.max(np.abs(gw - ow) / np.abs(ow)))
        elif o.counters()["n_minimizers"] != g.counters()["n_minimizers"]:
            ok = False; why = "minimizer counts differ"
        elif snap:
            # the trajectory: a second oracle, fed one spectrum's reads at a time (the last one may be ragged: the EOF flush)
            info, sm, sw = g.snapshots()
            step = interval if interval else len(seqs)
            want_reads = [min((t + 1) * step, len(seqs)) for t in range(n_spectra)]
            if [x["n_reads"] for x in info] != want_reads or [x["ordinal"] for x in info] != list(range(1, n_spectra + 1)):
                ok = False; why = f"snapshots recorded at {[(x['ordinal'], x['n_reads']) for x in info][:6]}..., expected reads {want_reads[:6]}..."
            else:
                o2 = pyorc.Sketcher(k, w, S, 0, decay, interval)
                for t in range(n_spectra):
                    o2.add_reads(bases, offsets[t * step:want_reads[t] + 1])
                    if t == n_spectra - 1:
                        o2.finish()
                    tm, tw = o2.sketch()
                    if not np.array_equal(tm, sm[t]):
                        ok = False; why = f"snapshot {t + 1} of {n_spectra}: {int((tm != sm[t]).sum())} of {S} mins differ"; break
                    if not np.allclose(sw[t], tw, rtol=1e-7 if decay != 1.0 else 1e-9, atol=0):
                        ok = False; why = f"snapshot {t + 1} of {n_spectra}: weights differ"; break
                o2.close()
    if oerr is not None:
        n_err += 1; errs[oerr] = errs.get(oerr, 0) + 1
    if not ok:
        bad += 1
        print("MISMATCH", desc, "::", why, flush=True)
        if only is not None or "FUZZ_FROM" in os.environ:      # diagnosis: which reads disagree on their number of distinct minimizers
            print("cuts", cuts, "oracle", o.counters(), "gpu", g.counters())
            for variant in ("same cuts", "one call", "NO_FAST"):
                if variant == "NO_FAST":
                    if not hulk_amd._lib.is_experiments_build():   # (the switch is compiled into the profiling build only)
                        print(" rerun NO_FAST: skipped — run with HULK_LIB=exp")
                        continue
                    os.environ["HULK_NO_FAST_K1"] = "1"
                g2 = hulk_amd.GpuSketcher(k, w, S, interval, decay, batch=batch, work_lanes=1 if variant == "one call" else lanes)
                try:
                    cc = cuts if variant == "same cuts" else [0, len(seqs)]
                    for x, y in zip(cc[:-1], cc[1:]):
                        g2.add_reads(bases, offsets[x:y + 1])
                    g2.finish()
                    print(" rerun", variant, g2.counters())
                except HulkError as e:
                    print(" rerun", variant, "error", e.message)
                g2.close()
                os.environ.pop("HULK_NO_FAST_K1", None)
            for x, y in zip(cuts[:-1], cuts[1:]):          # which call's reads disagree
                oo = pyorc.Sketcher(k, w, 1, 0, 1.0, 0); g3 = hulk_amd.GpuSketcher(k, w, 1)
                try:
                    oo.add_reads(bases, offsets[x:y + 1]); g3.add_reads(bases, offsets[x:y + 1])
                    ho, hg = oo.histogram(), g3.histogram()
                    print(" call", x, y, "maxlen", max(len(q) for q in seqs[x:y]) if y > x else 0, "oracle", oo.counters()["n_minimizers"], "gpu", g3.counters()["n_minimizers"], "hist equal", bool(np.array_equal(ho.astype(np.uint32), hg)))
                except Exception as e:
                    print(" call", x, y, "error", e)
                oo.close(); g3.close()
            for i, sq in enumerate(seqs):
                try:
                    no = len(pyorc.minimizers(sq, k, w))
                except pyorc.OracleError:
                    continue
                gg = hulk_amd.GpuSketcher(k, w, 1)
                gg.add_seq(sq)
                ng = gg.counters()["n_minimizers"]
                gg.close()
                if no != ng:
                    print("read", i, "len", len(sq), "oracle", no, "gpu alone", ng, sq[:80])
    g.close(); o.close()
print(f"{n_cases} cases ({n_cases - n_err} sketches compared, {n_err} agreed on an error: {errs}), {bad} mismatches, "
      f"{time.time() - t_start:.1f} s (seed {seed})")
sys.exit(1 if bad else 0)
