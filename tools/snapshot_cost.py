#!/usr/bin/env python3
"""What sketch snapshots cost a step (hulk_set_snapshots, GpuSketcher(snapshots=N)): profiles/snapshots.txt, sections 1-3.

Two configurations, both as bench.py runs them (synthetic 150-bp reads resident in HBM, hulk_add_reads_device, 16 intervals of
100,000 reads per step):
  C2  k = 21, sketchSize = 512, no decay       snapshots switch the scan and the resolve from the merged to the per-interval form
  C3  k = 31, sketchSize = 1024, decay 0.02     concept drift: the per-interval form is what runs anyway, snapshots add the stores
For each, snapshots off / every = 1 / every = 16 alternate in ONE process, `--rounds` times; every run is a fresh context and a
ramp of elementwise kernels (the chip's clocks).  Timed by the wall clock between two synchronisations:
  first    the first `--first` steps one by one (no batch is pruned or skipped yet: the full per-interval scan)
  steady   `--steps` steps after `--warmup` more (C2: k_flush_decide passes every batch over, one small copy kernel remains)
Section 2: the scan kernel alone (hulk_set_profiling bit 8) on a full pass — HULK_FLAG_NO_PRUNE | HULK_FLAG_NO_SKIP, every tile of
the table read in every step — merged (snapshots off) against per-interval (every = 1).
Section 3 (`--table`): hulk_get_profile_table over C2 steps of a context WITHOUT snapshots on one stream (HULK_FLAG_NO_OVERLAP,
profiling bit 32): kernel, launches.  `--root DIR` imports hulk_amd from another checkout — the parent commit's, whose table
has to list the same kernels with the same launch counts.

  python tools/snapshot_cost.py [--steps 20] [--warmup 3] [--first 2] [--rounds 3] [--configs C2,C3] [--modes off,every=1,every=16] [--out FILE]
  python tools/snapshot_cost.py --table [--root DIR]
"""
import argparse
import os
import statistics
import sys
import time

CONFIGS = {
    "C2": dict(k=21, w=9, S=512, decay=1.0, interval=100_000),
    "C3": dict(k=31, w=9, S=1024, decay=0.02, interval=100_000),
}
READ_LEN, BATCH, RAMP_MS = 150, 16, 40.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--first", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--modes", default="off,every=1,every=16", help="`off` alone also runs on a checkout without the feature (--root)")
    ap.add_argument("--table", action="store_true", help="section 3 only: the kernels of a C2 step without snapshots")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to import hulk_amd from (default: this one)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    import hulk_amd
    from hulk_amd import _lib, synth
    if not torch.cuda.is_available():
        raise SystemExit("snapshot_cost.py needs an MI355X")
    ramp_buf = torch.zeros(1 << 24, device="cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def make(cfg, every, flags=0):
        kw = dict(interval=cfg["interval"], decay_ratio=cfg["decay"], flags=flags, batch=BATCH)
        if every:
            kw.update(snapshots=every, snapshot_capacity=64)
        return hulk_amd.GpuSketcher(cfg["k"], cfg["w"], cfg["S"], **kw)

    def ramp():
        t_end = time.perf_counter() + RAMP_MS * 1e-3
        while time.perf_counter() < t_end:
            for _ in range(8):
                ramp_buf.sin_()
            torch.cuda.synchronize()

    def timed(sk, step, lo, hi):
        sk.synchronize(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(lo, hi):
            step(t)
        sk.synchronize(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / (hi - lo)

    build = _lib.load().hulk_build_info().decode()
    if a.table:
        cfg = CONFIGS["C2"]
        n_step = BATCH * cfg["interval"]
        bufs = [synth.reads_torch(i * n_step, n_step, READ_LEN)[0] for i in range(2)]
        offs = synth.reads_torch(0, n_step, READ_LEN)[1]
        sk = make(cfg, 0, _lib.HULK_FLAG_NO_OVERLAP)
        sk.set_profiling(32)
        for t in range(4):
            sk.add_reads_device(bufs[t % 2].data_ptr(), offs.data_ptr(), n_step, READ_LEN, bufs[t % 2].numel())
        tab = sk.profile_table()
        sk.close()
        say(f"# tools/snapshot_cost.py --table: C2, no snapshots, HULK_FLAG_NO_OVERLAP, 4 steps of {n_step} reads; {build}")
        say(f"  {'kernel':28s} {'launches':>8s} {'total ms':>10s}")
        for k in sorted(tab):
            say(f"  {k:28s} {tab[k][0]:8d} {tab[k][1]:10.3f}")
        say("  launches: " + " ".join(f"{k}={tab[k][0]}" for k in sorted(tab)))
    else:
        say(f"# tools/snapshot_cost.py: {READ_LEN}-bp synthetic reads in HBM, hulk_add_reads_device, {BATCH} intervals x 100,000 reads per step,")
        say(f"# first {a.first} steps one by one, then warm-up {a.warmup}, {a.steps} timed steps; wall clock between synchronisations; {build}")
        modes = tuple((m, int(m.split("=")[1]) if "=" in m else 0) for m in a.modes.split(","))
        for name in a.configs.split(","):
            cfg = CONFIGS[name]
            n_step = BATCH * cfg["interval"]
            bufs = [synth.reads_torch(i * n_step, n_step, READ_LEN)[0] for i in range(2)]
            offs = synth.reads_torch(0, n_step, READ_LEN)[1]
            torch.cuda.synchronize()
            first = {m: [[] for _ in range(a.first)] for m, _ in modes}
            steady = {m: [] for m, _ in modes}
            recorded = {}
            for r in range(a.rounds):
                for m, every in modes:
                    sk = make(cfg, every)
                    ramp()

                    def step(t, sk=sk):
                        b = bufs[t % 2]
                        sk.add_reads_device(b.data_ptr(), offs.data_ptr(), n_step, READ_LEN, b.numel())
                    for t in range(a.first):
                        first[m][t].append(timed(sk, step, t, t + 1))
                    timed(sk, step, a.first, a.first + a.warmup)
                    steady[m].append(timed(sk, step, a.first + a.warmup, a.first + a.warmup + a.steps))
                    if every:
                        recorded[m] = sk.snapshot_count()[0]
                    sk.close()
            say(f"\n{name}: k = {cfg['k']}, sketchSize = {cfg['S']}, decay {cfg['decay']}, {n_step} reads per step; ms per step over {a.rounds} alternating rounds (min / median)")
            say(f"  {'snapshots':10s} " + " ".join(f"{'step ' + str(t + 1):>17s}" for t in range(a.first)) + f" {'steady':>17s}   steady ratio to the first row   steady runs")
            b_min, b_med = min(steady[modes[0][0]]), statistics.median(steady[modes[0][0]])
            for m, _ in modes:
                cols = " ".join(f"{min(first[m][t]):8.3f}/{statistics.median(first[m][t]):8.3f}" for t in range(a.first))
                mn, md = min(steady[m]), statistics.median(steady[m])
                say(f"  {m:10s} {cols} {mn:8.3f}/{md:8.3f}   {mn / b_min:6.3f} / {md / b_med:6.3f}      " + " ".join(f"{x:.3f}" for x in steady[m])
                    + (f"   ({recorded[m]} snapshots recorded per run)" if m in recorded else ""))
            # section 2: the scan kernel alone, every tile read in every step
            full = _lib.HULK_FLAG_NO_PRUNE | _lib.HULK_FLAG_NO_SKIP
            say(f"  scan stage on a full pass (HULK_FLAG_NO_PRUNE | HULK_FLAG_NO_SKIP, the scan kernel's own brackets, {a.first + a.warmup} steps):")
            for m, every in modes[:2]:
                if every > 1:
                    continue
                sk = make(cfg, every, full)
                sk.set_profiling(8)
                ramp()
                for t in range(a.first + a.warmup):
                    b = bufs[t % 2]
                    sk.add_reads_device(b.data_ptr(), offs.data_ptr(), n_step, READ_LEN, b.numel())
                n, ms = sk.get_profile("k_cws_scan")
                form = "per interval" if (every or cfg["decay"] != 1.0) else "merged"
                say(f"    snapshots {m:8s} ({form:12s}): {n} launches, {ms / max(n, 1) * 1e3:9.1f} us each")
                sk.close()
            del bufs
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
