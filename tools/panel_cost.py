#!/usr/bin/env python3
"""What scoring every sketch snapshot against a panel costs a step (hulk_set_panel, GpuSketcher.set_panel): profiles/panel.txt.

The two configurations of tools/snapshot_cost.py, as bench.py runs them (synthetic 150-bp reads resident in HBM,
hulk_add_reads_device, 16 intervals of 100,000 reads per step), both with snapshots every = 1 (16 snapshots per flush):
  C2  k = 21, sketchSize = 512, no decay
  C3  k = 31, sketchSize = 1024, decay 0.02
For each, no panel / a panel of 1,024 / of 8,192 random sketches (weightedjaccard, role row) alternate in ONE process, `--rounds`
times; every run is a fresh context and a ramp of elementwise kernels (the chip's clocks).  Timed by the wall clock between two
synchronisations: the first `--first` steps one by one, then `--steps` steps after `--warmup` more.
Section 2: k_snap_panel alone — each (configuration, panel) in a child process under `rocprofv3 --kernel-trace --stats`, the
kernel's row of the statistics.

  python tools/panel_cost.py [--steps 20] [--warmup 3] [--first 2] [--rounds 3] [--configs C2,C3] [--panels 0,1024,8192] [--out FILE]
  python tools/panel_cost.py --child C2:1024          (what section 2 runs under rocprofv3)
"""
import argparse
import csv
import glob
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {
    "C2": dict(k=21, w=9, S=512, decay=1.0, interval=100_000),
    "C3": dict(k=31, w=9, S=1024, decay=0.02, interval=100_000),
}
READ_LEN, BATCH, RAMP_MS, CHILD_STEPS = 150, 16, 40.0, 6


def make(cfg, n_panel, flags=0):
    import numpy as np
    import hulk_amd
    sk = hulk_amd.GpuSketcher(cfg["k"], cfg["w"], cfg["S"], interval=cfg["interval"], decay_ratio=cfg["decay"], flags=flags, batch=BATCH,
                              snapshots=1, snapshot_capacity=64)
    if n_panel:
        rng = np.random.default_rng(n_panel)
        mins = rng.integers(0, min(cfg["k"] ** 4, 1 << 62), size=(n_panel, cfg["S"])).astype(np.uint64)
        sk.set_panel(mins, -rng.gamma(2.0, 1e-3, size=(n_panel, cfg["S"])), "weightedjaccard", "row")
    return sk


def child(spec):
    """a few steps of one configuration with one panel: the workload rocprofv3 traces"""
    sys.path.insert(0, ROOT)
    from hulk_amd import synth
    name, n_panel = spec.split(":")
    cfg = CONFIGS[name]
    n_step = BATCH * cfg["interval"]
    bases, offs = synth.reads_torch(0, n_step, READ_LEN)
    sk = make(cfg, int(n_panel))
    for _ in range(CHILD_STEPS):
        sk.add_reads_device(bases.data_ptr(), offs.data_ptr(), n_step, READ_LEN, bases.numel())
    sk.synchronize()
    print(f"child {spec}: {sk.snapshot_count()[0]} snapshots scored", flush=True)
    sk.close()


def traced(spec):
    """-> the lines of rocprofv3's kernel statistics that belong to k_snap_panel (header first).  A child that fails — an abort, a
    fault, a time limit, whatever — ends the tool: nothing more is started on a card a process has just failed on."""
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    with tempfile.TemporaryDirectory() as d:
        cmd = [tool, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", spec]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        except (OSError, subprocess.SubprocessError) as e:
            raise SystemExit(f"panel_cost.py: the traced run of {spec} did not finish ({e}); nothing more is started")
        if p.returncode != 0:
            raise SystemExit(f"panel_cost.py: the traced run of {spec} ended with status {p.returncode}; nothing more is started\n"
                             + (p.stderr or p.stdout)[-2000:])
        out = []
        for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            rows = list(csv.reader(open(f)))
            if not rows:
                continue
            head = {h: i for i, h in enumerate(rows[0])}
            for r in rows[1:]:
                if r and "k_snap_panel" in r[0]:
                    if all(h in head for h in ("Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs")):
                        out.append(f"{(re.search(r'k_snap_panel<[^>]*>', r[0]) or re.search(r'.+', r[0])).group(0):24s} calls {int(r[head['Calls']]):4d}  total {float(r[head['TotalDurationNs']]) / 1e3:10.1f} us  "
                                   f"average {float(r[head['AverageNs']]) / 1e3:8.1f} us  min {float(r[head['MinNs']]) / 1e3:8.1f}  max {float(r[head['MaxNs']]) / 1e3:8.1f}")
                    else:
                        out.append(",".join(rows[0])); out.append(",".join(r))
        return out or ["(no k_snap_panel row in rocprofv3's kernel statistics)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--first", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--panels", default="0,1024,8192")
    ap.add_argument("--no-trace", action="store_true", help="skip section 2 (the rocprofv3 runs)")
    ap.add_argument("--child", default="", help="CONFIG:PANEL — run the traced workload and exit")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    panels = [int(x) for x in a.panels.split(",")]
    # section 2 first: its children are started before this process opens the GPU
    trace = {}
    if not a.no_trace:
        for name in a.configs.split(","):
            for n_panel in panels:
                if n_panel:
                    trace[name, n_panel] = traced(f"{name}:{n_panel}")
    sys.path.insert(0, ROOT)
    import torch
    from hulk_amd import _lib, synth
    if not torch.cuda.is_available():
        raise SystemExit("panel_cost.py needs an MI355X")
    ramp_buf = torch.zeros(1 << 24, device="cuda")

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
    say(f"# tools/panel_cost.py: {READ_LEN}-bp synthetic reads in HBM, hulk_add_reads_device, {BATCH} intervals x 100,000 reads per step, snapshots every = 1,")
    say(f"# first {a.first} steps one by one, then warm-up {a.warmup}, {a.steps} timed steps; wall clock between synchronisations; {build}")
    for name in a.configs.split(","):
        cfg = CONFIGS[name]
        n_step = BATCH * cfg["interval"]
        bufs = [synth.reads_torch(i * n_step, n_step, READ_LEN)[0] for i in range(2)]
        offs = synth.reads_torch(0, n_step, READ_LEN)[1]
        torch.cuda.synchronize()
        first = {p: [[] for _ in range(a.first)] for p in panels}
        steady = {p: [] for p in panels}
        for r in range(a.rounds):
            for n_panel in panels:
                sk = make(cfg, n_panel)
                ramp()

                def step(t, sk=sk):
                    b = bufs[t % 2]
                    sk.add_reads_device(b.data_ptr(), offs.data_ptr(), n_step, READ_LEN, b.numel())
                for t in range(a.first):
                    first[n_panel][t].append(timed(sk, step, t, t + 1))
                timed(sk, step, a.first, a.first + a.warmup)
                steady[n_panel].append(timed(sk, step, a.first + a.warmup, a.first + a.warmup + a.steps))
                sk.close()
        say(f"\n{name}: k = {cfg['k']}, sketchSize = {cfg['S']}, decay {cfg['decay']}, {n_step} reads per step; ms per step over {a.rounds} alternating rounds (min / median)")
        say(f"  {'panel':10s} " + " ".join(f"{'step ' + str(t + 1):>17s}" for t in range(a.first)) + f" {'steady':>17s}   steady ratio to the first row   steady runs")
        b_min, b_med = min(steady[panels[0]]), statistics.median(steady[panels[0]])
        for n_panel in panels:
            cols = " ".join(f"{min(first[n_panel][t]):8.3f}/{statistics.median(first[n_panel][t]):8.3f}" for t in range(a.first))
            mn, md = min(steady[n_panel]), statistics.median(steady[n_panel])
            label = f"P={n_panel}" if n_panel else "none"
            say(f"  {label:10s} {cols} {mn:8.3f}/{md:8.3f}   {mn / b_min:6.3f} / {md / b_med:6.3f}      " + " ".join(f"{x:.3f}" for x in steady[n_panel]))
        spread = max(steady[panels[0]]) - min(steady[panels[0]])
        say(f"  run-to-run spread of the panel-less leg: {spread:.3f} ms")
        for n_panel in panels[1:]:
            over = statistics.median(steady[n_panel]) - b_med
            say(f"  P={n_panel}: median steady step {over:+.3f} ms against no panel ({'within' if over <= spread else 'ABOVE'} that spread)")
        if trace:
            say(f"  k_snap_panel alone (rocprofv3 --kernel-trace --stats, {CHILD_STEPS} steps = {CHILD_STEPS} launches of 16 snapshots, a process each):")
            for n_panel in panels:
                for ln in trace.get((name, n_panel), []):
                    say(f"    P={n_panel}: {ln}")
        del bufs
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
