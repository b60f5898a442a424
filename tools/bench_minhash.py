#!/usr/bin/env python3
"""What feeding the MinHash sketches costs a steady-state step (HULK_FLAG_KMV / HULK_FLAG_KHF): profiles/minhash.txt.

Two configurations, both as bench.py runs them (synthetic 150-bp reads resident in HBM, hulk_add_reads_device, 16 intervals of
100,000 reads per step):
  C2  k = 21, sketchSize = 512, no decay       KHF is the exact min-reduction (2k + 8 + log2 S <= 64: no product wraps)
  C3  k = 31, sketchSize = 1024, decay 0.02     KHF is brute force: every value updates every slot
For each, flags 0 / KMV / KHF / KMV|KHF alternate in ONE process, `--rounds` times; every run is a fresh context, a ramp of
elementwise kernels (the chip's clocks), `--warmup` steps, then `--steps` steps timed by the wall clock between two
synchronisations.  Prints min and median ms per step and the ratio to flags 0, and checks once per configuration that the
signatures of the KMV|KHF run are those of a second, differently batched context (order independence).

  python tools/bench_minhash.py [--steps 20] [--warmup 3] [--rounds 3] [--configs C2,C3] [--out profiles/minhash.txt]
  python tools/bench_minhash.py --one C2:3 --steps 20       one KMV|KHF run and nothing else (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "C2": dict(k=21, w=9, S=512, decay=1.0, interval=100_000),
    "C3": dict(k=31, w=9, S=1024, decay=0.02, interval=100_000),
}
READ_LEN, BATCH, RAMP_MS = 150, 16, 40.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--one", default="", help="<config>:<flag mask 0..3>: a single run (bit 0 KMV, bit 1 KHF)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import hulk_amd
    from hulk_amd import _lib, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_minhash.py needs an MI355X")
    names = ("0", "KMV", "KHF", "KMV|KHF")
    masks = (0, _lib.HULK_FLAG_KMV, _lib.HULK_FLAG_KHF, _lib.HULK_FLAG_KMV | _lib.HULK_FLAG_KHF)
    ramp_buf = torch.zeros(1 << 24, device="cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def run(cfg, flags, bufs, offs, n_step, steps, keep=False):
        sk = hulk_amd.GpuSketcher(cfg["k"], cfg["w"], cfg["S"], interval=cfg["interval"], decay_ratio=cfg["decay"], flags=flags, batch=BATCH)
        t_end = time.perf_counter() + RAMP_MS * 1e-3
        while time.perf_counter() < t_end:
            for _ in range(8):
                ramp_buf.sin_()
            torch.cuda.synchronize()
        def step(t):
            b = bufs[t % len(bufs)]
            sk.add_reads_device(b.data_ptr(), offs.data_ptr(), n_step, READ_LEN, b.numel())
        for t in range(a.warmup):
            step(t)
        sk.synchronize(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(a.warmup, a.warmup + steps):
            step(t)
        sk.synchronize(); torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        sig = None
        if keep:
            sig = (sk.minhash(_lib.HULK_MINHASH_KMV), sk.minhash(_lib.HULK_MINHASH_KHF))
        sk.close()
        return ms, sig

    say(f"# tools/bench_minhash.py: {READ_LEN}-bp synthetic reads in HBM, hulk_add_reads_device, {BATCH} intervals x 100,000 reads per step,")
    say(f"# warm-up {a.warmup} steps, {a.steps} timed steps per run, wall clock between synchronisations; {hulk_amd._lib.load().hulk_build_info().decode()}")
    todo = [a.one.split(":")[0]] if a.one else a.configs.split(",")
    for name in todo:
        cfg = CONFIGS[name]
        n_step = BATCH * cfg["interval"]
        bufs = [synth.reads_torch(i * n_step, n_step, READ_LEN)[0] for i in range(2)]
        offs = synth.reads_torch(0, n_step, READ_LEN)[1]
        torch.cuda.synchronize()
        if a.one:
            ms, _ = run(cfg, masks[int(a.one.split(":")[1])], bufs, offs, n_step, a.steps)
            say(f"{name} flags {names[int(a.one.split(':')[1])]}: {ms:.3f} ms per step")
            continue
        times = {n: [] for n in names}
        for r in range(a.rounds):
            for n, m in zip(names, masks):
                ms, _ = run(cfg, m, bufs, offs, n_step, a.steps)
                times[n].append(ms)
        say(f"\n{name}: k = {cfg['k']}, sketchSize = {cfg['S']}, decay {cfg['decay']}, {n_step} reads per step; ms per step over {a.rounds} alternating rounds")
        say(f"  {'flags':8s} {'min':>9s} {'median':>9s}   ratio to flags 0 (min / median)   runs")
        base_min, base_med = min(times["0"]), statistics.median(times["0"])
        for n in names:
            mn, md = min(times[n]), statistics.median(times[n])
            say(f"  {n:8s} {mn:9.3f} {md:9.3f}   {mn / base_min:6.3f} / {md / base_med:6.3f}                  " + " ".join(f"{x:.3f}" for x in times[n]))
        # the same stream, two steps, batched differently: identical signatures
        _, s1 = run(cfg, masks[3], bufs, offs, n_step, 2, keep=True)
        sk = hulk_amd.GpuSketcher(cfg["k"], cfg["w"], cfg["S"], interval=cfg["interval"] // 4, decay_ratio=cfg["decay"], flags=masks[3], batch=4, work_lanes=1)
        for t in range(a.warmup + 2):
            b = bufs[t % 2]
            for piece in range(4):
                lo = piece * (n_step // 4)
                sk.add_reads_device(b.data_ptr() + lo * READ_LEN, offs.data_ptr(), n_step // 4, READ_LEN, b.numel() - lo * READ_LEN)
        s2 = (sk.minhash(_lib.HULK_MINHASH_KMV), sk.minhash(_lib.HULK_MINHASH_KHF))
        sk.close()
        same = all((x[0] == y[0]).all() and x[1] == y[1] for x, y in zip(s1, s2))
        say(f"  signatures of a second context fed the same {(a.warmup + 2) * n_step} reads in quarter steps on one lane: {'identical' if same else 'DIFFERENT'} ({s1[0][1]} values fed)")
        if not same:
            raise SystemExit("bench_minhash.py: signatures differ")
        del bufs
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
