#!/usr/bin/env python3
"""k_minimizer_fast's PAIR instance (two 16-lane groups per read) on its own workload: 0.8 M synthetic reads of 300 bases, resident
in HBM, binned --steps times at k = 21, w = 9.  The driver only runs the work; the kernel's time per launch comes from a kernel
trace around it, with every kernel alone:

  HULK_LIB=exp HULK_NO_OVERLAP=1 rocprofv3 --kernel-trace --stats -d OUT -o p -- python tools/k1_pair_workload.py

HULK_LIB=<path> selects another build of the library (the parent's, for an A/B); HULK_K1_LDS_TOTAL=<bytes> (profiling build) pads the
kernel's LDS request, which steps its workgroups per CU down: 31968 -> 5, 40928 -> 4, 53728 -> 3 (see profiles/k1a_occupancy.md).
Prints one JSON line: reads, bases, wall time per step (all kernels of the step, not the figure to quote) and the minimizer count."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=800_000)
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    import hulk_amd
    from hulk_amd import synth
    b, off = synth.reads_torch(0, a.reads, a.length)
    torch.cuda.synchronize()
    g = hulk_amd.GpuSketcher(21, 9, 50)
    try:
        t0 = 0.0
        for s in range(a.warmup + a.steps):
            if s == a.warmup:
                g.synchronize(); t0 = time.perf_counter()
            g.add_reads_device(b.data_ptr(), off.data_ptr(), a.reads, a.length, b.numel())
        g.synchronize()
        dt = time.perf_counter() - t0
        c = g.counters()
        print(json.dumps({"reads": a.reads, "length": a.length, "steps": a.steps, "ms_per_step_wall": dt / a.steps * 1e3,
                          "n_minimizers": int(c["n_minimizers"]), "lib": os.environ.get("HULK_LIB", ""),
                          "lds_total": os.environ.get("HULK_K1_LDS_TOTAL", "")}))
    finally:
        g.close()


if __name__ == "__main__":
    main()
