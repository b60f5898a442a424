#!/usr/bin/env python3
"""What a complete- or average-linkage dendrogram costs (hulk_linkage: the matrix kernel + k_linkage_sym, then k_linkage_pick,
k_linkage_update and k_linkage_rescan per merge): profiles/linkage.txt.

N sketches (default 4,096, 16,384 and 32,768) at S = 512, jaccard and weightedjaccard, on tools/cluster_cost.py's sets.  Per cell,
in one process:
  the matrix phase (kernel_ms_matrix: hulk_smash's kernel and k_linkage_sym) next to hulk_smash_ex's kernel_ms at the same N;
  the merge phase (kernel_ms_merge) as microseconds per merge, and rows_rescanned / merges, for every method;
  the floor of the merge phase: the same call on a set whose weights are all zero under weightedjaccard — every pair is NaN, the first
  pick finds nothing, and the rest of the first chunk (4,096 merges of three launches each, the same grids) returns at once:
  kernel_ms_merge / the merges queued is what the launches alone cost on this machine;
  where SciPy is installed and N is at most --scipy-max-n: the wall time of scipy.cluster.hierarchy.linkage(squareform(W), method) on
  the host for the same set (the matrix pulled to the host with hulk_smash first, which is not counted).

  python tools/linkage_rate.py [--n 4096,16384,32768] [--s 512] [--methods complete,average] [--scipy-max-n 16384] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CHUNK = 4096                                                    # hulk_linkage.hip's LINK_CHUNK: merges queued between two looks at "finished"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="4096,16384,32768")
    ap.add_argument("--s", type=int, default=512)
    ap.add_argument("--methods", default="complete,average")
    ap.add_argument("--scipy-max-n", type=int, default=16384)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    from cluster_cost import sketches
    from hulk_amd import _lib, smash
    out = open(a.out, "w") if a.out else None

    def say(line=""):
        print(line, flush=True)
        if out:
            out.write(line + "\n"); out.flush()

    try:
        from scipy.cluster import hierarchy
        from scipy.spatial.distance import squareform
        import scipy
        scipy_version = scipy.__version__
    except ImportError:
        hierarchy = None
        scipy_version = "not installed"
    L = _lib.load()
    say(f"# tools/linkage_rate.py: S = {a.s}; {L.hulk_build_info().decode()}; SciPy {scipy_version}")
    N_list = [int(x) for x in a.n.split(",")]
    methods = a.methods.split(",")
    s = a.s
    rng = np.random.default_rng(s)
    base = rng.integers(0, 194481, size=s).astype(np.uint64)
    m_all, w_all = sketches(rng, max(N_list), s, base)
    smash.linkage(m_all[:256], w_all[:256], "complete", "jaccard"); smash.linkage(m_all[:256], w_all[:256], "average", "weightedjaccard")     # (code load)
    for n in N_list:
        m, w = m_all[:n], w_all[:n]
        say()
        say(f"== N = {n} ({8 * n * n / 2 ** 30:.2f} GiB of matrix)")
        # the floor: nothing merges, the first chunk's launches return at once
        st = {}
        smash.linkage(m, np.zeros_like(w), "complete", "weightedjaccard", stats=st)
        queued = min(CHUNK, n - 1)
        assert st["merges"] == 0
        say(f"  empty launches: {queued} merges queued (3 launches each: 1, {(n + 255) // 256} and {(n + 15) // 16} workgroups), nothing to merge: "
            f"kernel_ms_merge {st['kernel_ms_merge']:.3f} ms = {1e3 * st['kernel_ms_merge'] / queued:.2f} us a merge (the first fill of the cache and one full pick included)")
        for metric in ("jaccard", "weightedjaccard"):
            tm = {}
            runs = 3 if n <= 16384 else 1
            ms = []
            for _ in range(runs):
                D = smash.distance_matrix(m, w, metric, timing=tm)
                ms.append(tm["kernel_ms"])
            say(f"  {metric}: hulk_smash_ex kernel_ms: " + " ".join(f"{x:.3f}" for x in ms))
            for method in methods:
                st = {}
                t0 = time.perf_counter()
                ga, gb, gd, gs = smash.linkage(m, w, method, metric, stats=st)
                wall = time.perf_counter() - t0
                k = max(st["merges"], 1)
                say(f"  {metric} {method}: {st['merges']} merges, {st['components']} cluster(s) left; matrix phase {st['kernel_ms_matrix']:.3f} ms "
                    f"= {st['kernel_ms_matrix'] / min(ms):.3f} x hulk_smash_ex; merge phase {st['kernel_ms_merge']:.3f} ms = {1e3 * st['kernel_ms_merge'] / k:.2f} us a merge; "
                    f"rows_rescanned / merges {(st['rows_rescanned'] - n) / k:.2f} (the first fill's {n} rows left out); the call {st['seconds_total']:.3f} s ({wall:.3f} s from Python); "
                    f"heights {float(gd[0])!r} .. {float(gd.max())!r}")
            if hierarchy is not None and n <= a.scipy_max_n:
                W = np.fmin(D, D.T)
                del D
                np.fill_diagonal(W, 0.0)
                if np.isnan(W).any():
                    say(f"  {metric}: SciPy skipped: NaN distances")
                    continue
                y = squareform(W, checks=False)
                del W
                for method in methods:
                    t0 = time.perf_counter()
                    Z = hierarchy.linkage(y, method=method)
                    say(f"  {metric} {method}: scipy.cluster.hierarchy.linkage on the host: {time.perf_counter() - t0:.3f} s (heights {Z[0, 2]!r} .. {Z[-1, 2]!r})")
                del y
            else:
                del D
                say(f"  {metric}: SciPy not run at this N" if hierarchy is not None else f"  {metric}: SciPy is not installed")
    L.hulk_release_caches()
    if out:
        out.close()


if __name__ == "__main__":
    main()
