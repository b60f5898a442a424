#!/usr/bin/env python3
"""What single-linkage clustering costs (hulk_cluster: k_cluster_link, k_cluster_flatten): profiles/cluster.txt.

N sketches (default 8,192 and 65,536) at S = 512 and S = 50, both metrics, at three link densities: tau = 0 (below every distance
of these sets: no link, no union — the tile's own cost), tau at the 1 % quantile of the distances (sparse links; estimated from the
first 1,024 sketches with hulk_smash_ex) and tau = 1 (every pair links: the union path's worst case).  kernel_ms_link from the
library's HIP events, summed over the bands, as pair-slots per second: the pair-slots actually computed — N x N x S for
weightedjaccard, the tiles on and above the diagonal for jaccard (k_cluster_link leaves the others at once).  In the same process,
before and after, `--smash-runs` runs of hulk_smash_ex over `--smash-n` sketches at the same S and as many `--self` searches
(k_search_dist): their pair-slots per second, the run-to-run spread, and the ratio to them.
Section 2: band_rows 512 / 1,536 / 1,600 / 2,048 / N (one band) at the first N and tau = 0: what the band launches cost (at
N = 8,192 a weighted band of 1,536 or 2,048 rows is a whole number of rounds of the 512 workgroups the chip holds, one of 1,600 is not).
Section 3 (needs the profiling build: HULK_LIB=exp): tau = 1 and the 1 % quantile, at the first N and S and at the last ones, with
and without the plain-load filter (HULK_CLUSTER_NO_FILTER) and a flatten behind every band (HULK_CLUSTER_BAND_FLATTEN; the library
flattens once, behind the last band).
A case whose distance work alone is estimated above `--budget-s` seconds is skipped and said so.

  python tools/cluster_cost.py [--n 8192,65536] [--s 512,50] [--smash-n 8192] [--smash-runs 5] [--budget-s 60] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sketches(rng, n, s, base):
    import numpy as np
    keep = rng.random((n, 1)) * 0.6 + 0.2 > rng.random((n, s))
    mins = np.where(keep, base[None, :], rng.integers(0, 194481, size=(n, s)).astype(np.uint64))
    return np.ascontiguousarray(mins), -rng.gamma(2.0, 1e-3, size=(n, s))


def pair_slots(n, s, metric, band=2048):
    """what k_cluster_link computes: jaccard keeps the 32 x 64 tiles that hold a pair s < q"""
    if metric == "weightedjaccard":
        return n * n * s
    np64 = (n + 63) // 64 * 64
    tiles = 0
    for s0 in range(0, n, 32):
        first = (s0 - s0 % band) // 64                      # tiles in front of the band's first row are not launched
        tiles += sum(1 for qt in range(first, np64 // 64) if s0 < qt * 64 + 63)
    return tiles * 32 * 64 * s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="8192,65536")
    ap.add_argument("--s", default="512,50")
    ap.add_argument("--smash-n", type=int, default=8192)
    ap.add_argument("--smash-runs", type=int, default=5)
    ap.add_argument("--budget-s", type=float, default=60.0)
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
    say(f"# tools/cluster_cost.py: default band_rows (2048); {info}")
    N_list, S_list = [int(x) for x in a.n.split(",")], [int(x) for x in a.s.split(",")]
    guess = {"jaccard": 9e12, "weightedjaccard": 5e12}      # pair-slots/s of k_smash, for the budget only

    def cluster_runs(m, w, tau, metric, runs, band_rows=0):
        got = []
        for _ in range(runs):
            st = {}
            smash.cluster(m, w, tau, metric, band_rows=band_rows, stats=st)
            got.append(st)
        return got

    for s in S_list:
        rng = np.random.default_rng(s)
        base = rng.integers(0, 194481, size=s).astype(np.uint64)
        m_all, w_all = sketches(rng, max(max(N_list), a.smash_n), s, base)
        say()
        say(f"== S = {s}")

        def reference(metric):
            """-> the median pair-slots per second of hulk_smash_ex and of a --self search, and their spreads"""
            sm, se = [], []
            smash.distance_matrix(m_all[:256], w_all[:256], metric)              # (code load)
            smash.search(m_all[:256], w_all[:256], None, None, 10, metric, self_search=True)
            for _ in range(a.smash_runs):
                t = {}
                smash.distance_matrix(m_all[:a.smash_n], w_all[:a.smash_n], metric, timing=t)
                sm.append(a.smash_n * a.smash_n * s / (t["kernel_ms"] * 1e-3))
            for _ in range(a.smash_runs):
                st = {}
                smash.search(m_all[:a.smash_n], w_all[:a.smash_n], None, None, 10, metric, self_search=True, stats=st)
                se.append(a.smash_n * a.smash_n * s / (st["kernel_ms_dist"] * 1e-3))
            return sm, se

        for metric in ("jaccard", "weightedjaccard"):
            say(f"  {metric}")
            sm, se = reference(metric)
            med_sm, med_se = statistics.median(sm), statistics.median(se)
            say(f"    hulk_smash_ex N = {a.smash_n}: " + " ".join(f"{x:.4g}" for x in sm) + f"  -> median {med_sm:.4g} pair-slots/s, spread {100 * (max(sm) - min(sm)) / med_sm:.1f} %")
            say(f"    search --self N = {a.smash_n}: " + " ".join(f"{x:.4g}" for x in se) + f"  -> median {med_se:.4g} pair-slots/s, spread {100 * (max(se) - min(se)) / med_se:.1f} %")
            D = smash.distance_matrix(m_all[:1024], w_all[:1024], metric)
            off = D[~np.eye(1024, dtype=bool)]
            q1 = float(np.quantile(off[~np.isnan(off)], 0.01))
            say(f"    {'N':>7} {'tau':>10} {'runs':>4} {'bands':>5} {'link ms':>10} {'flatten ms':>10} {'links':>14} {'clusters':>8} {'pair-slots/s':>13} {'vs k_smash':>10} {'vs search':>9} {'end to end s':>13}")
            smash.cluster(m_all[:256], w_all[:256], 0.5, metric)                 # (code load)
            for n in N_list:
                work = pair_slots(n, s, metric)
                if work / guess[metric] > a.budget_s:
                    say(f"    {n:>7} skipped: {work:.3g} pair-slots, about {work / guess[metric]:.0f} s a run, above --budget-s {a.budget_s:g}")
                    continue
                runs = 3 if work / guess[metric] < 5 else 1
                for name, tau in (("0", 0.0), (f"{q1:.4f}", q1), ("1", 1.0)):
                    got = cluster_runs(m_all[:n], w_all[:n], tau, metric, runs)
                    best = min(got, key=lambda x: x["kernel_ms_link"])
                    rate = work / (best["kernel_ms_link"] * 1e-3)
                    if tau == 0.0 and best["links"]:
                        say(f"    (the set holds identical pairs: the next line is NOT a run without links)")
                    say(f"    {n:>7} {name:>10} {runs:>4} {best['bands']:>5} {best['kernel_ms_link']:>10.3f} {best['kernel_ms_flatten']:>10.3f} {best['links']:>14} {best['clusters']:>8} "
                        f"{rate:>13.4g} {rate / med_sm:>10.3f} {rate / med_se:>9.3f} {min(x['seconds_total'] for x in got):>13.4f}"
                        + ("   (all runs, link ms: " + " ".join(f"{x['kernel_ms_link']:.3f}" for x in got) + ")" if runs > 1 else ""))
            sm2, se2 = reference(metric)
            say(f"    again: hulk_smash_ex median {statistics.median(sm2):.4g}, search --self median {statistics.median(se2):.4g} pair-slots/s")
    # section 2: the band.  A band is one launch of k_cluster_link (for jaccard a staircase of tiles, the workgroups below the
    # diagonal leave at once), bracketed by its own events
    n = N_list[0]
    say()
    say(f"== band_rows at N = {n}, tau = 0 (three runs each, the fastest)")
    say(f"    {'S':>5} {'metric':>16} {'band_rows':>9} {'bands':>5} {'link ms':>10} {'flatten ms':>10} {'pair-slots/s':>13}")
    for s in S_list:
        rng = np.random.default_rng(s)
        base = rng.integers(0, 194481, size=s).astype(np.uint64)
        m, w = sketches(rng, n, s, base)
        for metric in ("jaccard", "weightedjaccard"):
            for band in (512, 1536, 1600, 2048, (n + 31) // 32 * 32):
                best = min(cluster_runs(m, w, 0.0, metric, 3, band), key=lambda x: x["kernel_ms_link"])
                say(f"    {s:>5} {metric:>16} {band:>9} {best['bands']:>5} {best['kernel_ms_link']:>10.3f} {best['kernel_ms_flatten']:>10.3f} "
                    f"{pair_slots(n, s, metric, band) / (best['kernel_ms_link'] * 1e-3):>13.4g}")
    # section 3: what the filter and the flatten behind every band are worth where links are dense
    say()
    if "experiments=1" not in info:
        say("== filter / flatten behind every band: not measured (the switches exist in the profiling build only: HULK_LIB=exp)")
    else:
        for n, s in ((N_list[0], S_list[0]), (N_list[-1], S_list[-1])):
            rng = np.random.default_rng(s)
            base = rng.integers(0, 194481, size=s).astype(np.uint64)
            m, w = sketches(rng, n, s, base)
            say(f"== filter / flatten behind every band at N = {n}, S = {s} (three runs each, the fastest by link ms + flatten ms)")
            say(f"    {'metric':>16} {'tau':>8} {'filter':>6} {'band flatten':>12} {'link ms':>10} {'flatten ms':>10} {'links':>14} {'clusters':>8}")
            for metric in ("jaccard", "weightedjaccard"):
                D = smash.distance_matrix(m[:1024], w[:1024], metric)
                off = D[~np.eye(1024, dtype=bool)]
                q1 = float(np.quantile(off[~np.isnan(off)], 0.01))
                for tau in (1.0, q1):
                    for filt in (True, False):
                        for flat in (True, False):
                            for key, switch in (("HULK_CLUSTER_NO_FILTER", not filt), ("HULK_CLUSTER_BAND_FLATTEN", flat)):
                                if switch:
                                    os.environ[key] = "1"
                                else:
                                    os.environ.pop(key, None)
                            got = cluster_runs(m, w, tau, metric, 3)
                            best = min(got, key=lambda x: x["kernel_ms_link"] + x["kernel_ms_flatten"])
                            say(f"    {metric:>16} {tau:>8.4f} {'on' if filt else 'off':>6} {'on' if flat else 'off':>12} {best['kernel_ms_link']:>10.3f} {best['kernel_ms_flatten']:>10.3f} "
                                f"{best['links']:>14} {best['clusters']:>8}")
            os.environ.pop("HULK_CLUSTER_NO_FILTER", None); os.environ.pop("HULK_CLUSTER_BAND_FLATTEN", None)
    L.hulk_release_caches()
    if out:
        out.close()


if __name__ == "__main__":
    main()
