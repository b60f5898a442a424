#!/usr/bin/env python3
"""What the bottom-k metric costs (HULK_METRIC_BOTTOMK: k_bottomk_prep, k_bottomk_matrix): profiles/bottomk.txt.

The matrix form (hulk_smash_ex) at N = 8,192 with S = 512 and at N = 1,024 with S = 2,048, on sets of KMV-like sketches (every
sketch S distinct values out of a pool of 4 S random uint64, so a pair shares about a quarter).  Per shape, `--rounds` rounds that
alternate, in one process,
  jaccard           k_smash_prep + k_smash over the same values (position by position: the number to compare with)
  bottomk           k_bottomk_prep + k_bottomk_matrix, the tile of hulk_bottomk_tile.h
  bottomk, global   k_bottomk_prep + k_bottomk_global: a thread a pair, merging the prepared lists where they lie in global memory —
                    the obvious fallback, the number to beat (HULK_BOTTOMK_GLOBAL=1)
  prep alone        k_bottomk_prep (HULK_BOTTOMK_GLOBAL=2)
each timed by the library's HIP events around its kernels (kernel_ms of hulk_smash_ex: preparation and matrix kernel, no copies).
The last two exist in the profiling build only (HULK_LIB=exp); without it they are "not measured".  Reported: every round, the
median, the spread, pair-values per second (N x N x S over the median), and the ratios of the medians.  The two bottomk variants
must give the same matrix, which is checked.

  HULK_LIB=exp python tools/profile_bottomk.py [--shapes 8192x512,1024x2048] [--rounds 5] [--out profiles/bottomk.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kmv_like(rng, n, s):
    import numpy as np
    pool = rng.integers(0, 2 ** 63, size=4 * s, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=4 * s, dtype=np.uint64)
    pool = np.unique(pool)
    pick = np.argsort(rng.random((n, len(pool))), axis=1)[:, :s]
    return np.sort(pool[pick], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x512,1024x2048")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    from hulk_amd import _lib, smash
    out = open(a.out, "w") if a.out else None

    def say(line=""):
        print(line, flush=True)
        if out:
            out.write(line + "\n"); out.flush()

    L = _lib.load()
    info = L.hulk_build_info().decode()
    exp = "experiments=1" in info
    say(f"# tools/profile_bottomk.py: {info}")
    say("# kernel_ms of hulk_smash_ex (HIP events around the preparation and the matrix kernel; no copies), every round, alternating")

    def timed(m, w, metric, mode):
        if mode:
            os.environ["HULK_BOTTOMK_GLOBAL"] = str(mode)
        else:
            os.environ.pop("HULK_BOTTOMK_GLOBAL", None)
        t = {}
        D = smash.distance_matrix(m, w, metric, timing=t)
        os.environ.pop("HULK_BOTTOMK_GLOBAL", None)
        return t["kernel_ms"], D

    for shape in a.shapes.split(","):
        n, s = (int(x) for x in shape.split("x"))
        rng = np.random.default_rng(n + s)
        m = kmv_like(rng, n, s)
        w = np.zeros(m.shape)
        legs = [("jaccard", "jaccard", 0), ("bottomk", "bottomk", 0)]
        if exp:
            legs += [("bottomk, global", "bottomk", 1), ("prep alone", "bottomk", 2)]
        say()
        say(f"== N = {n}, S = {s}: {n * n * s:.4g} pair-values")
        for name, metric, mode in legs:                             # (code load, buffers)
            timed(m[:256], w[:256], metric, mode)
        ms = {name: [] for name, _, _ in legs}
        keep = {}
        for r in range(a.rounds):
            for name, metric, mode in legs:
                t, D = timed(m, w, metric, mode)
                ms[name].append(t)
                if r == 0 and mode != 2:
                    keep[name] = D
        med = {k: statistics.median(v) for k, v in ms.items()}
        for name, _, _ in legs:
            v = ms[name]
            rate = "" if name == "prep alone" else f", {n * n * s / (med[name] * 1e-3):.4g} pair-values/s"
            say(f"  {name:<16} ms: " + " ".join(f"{x:.3f}" for x in v) + f"  -> median {med[name]:.3f}, spread {100 * (max(v) - min(v)) / med[name]:.1f} %{rate}")
        say(f"  bottomk / jaccard: {med['bottomk'] / med['jaccard']:.3f}")
        if exp:
            same = np.array_equal(keep["bottomk"].view(np.uint64), keep["bottomk, global"].view(np.uint64))
            say(f"  bottomk, global / bottomk: {med['bottomk, global'] / med['bottomk']:.3f}   (the two matrices are {'the same bits' if same else 'DIFFERENT'})")
            say(f"  the matrix kernel alone (median less the preparation's): tile {med['bottomk'] - med['prep alone']:.3f} ms, global {med['bottomk, global'] - med['prep alone']:.3f} ms")
            if not same:
                sys.exit("the tile and the merge from global memory disagree")
        else:
            say("  bottomk, global and prep alone: not measured (the switches exist in the profiling build only: HULK_LIB=exp)")
        off = keep["bottomk"][~np.eye(n, dtype=bool)]
        say(f"  (bottomk distances of the set: min {off.min():.4f}, median {np.median(off):.4f}, max {off.max():.4f}; jaccard median {np.median(keep['jaccard']):.4f})")
    L.hulk_release_caches()
    if out:
        out.close()


if __name__ == "__main__":
    main()
