#!/usr/bin/env python3
"""What the single-linkage dendrogram costs (hulk_dendrogram: k_dendro_offer, k_dendro_fold): profiles/dendrogram.txt.

N sketches (default 8,192 and 65,536) at S = 512 and S = 50, both metrics, on tools/cluster_cost.py's sets.  Per cell, in one
process: `--cluster-runs` runs of hulk_cluster at tau = 0 (kernel_ms_link: the no-link pass of the same tile over the same set),
the dendrogram (`--runs` runs: rounds, k_dendro_offer and k_dendro_fold summed over the rounds from the library's HIP events, end to
end seconds), the cluster leg again.  The figure compared is k_dendro_offer PER ROUND against the median kernel_ms_link; the
cluster leg's own run-to-run spread is printed beside it.  With the profiling build (HULK_LIB=exp) the first round — the dense
worst case: every pair offers — is also timed alone (HULK_DENDRO_ROUNDS=1).
A cell whose distance work alone is estimated above `--budget-s` seconds is skipped and said so.

  python tools/dendrogram_cost.py [--n 8192,65536] [--s 512,50] [--runs 3] [--cluster-runs 5] [--budget-s 60] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="8192,65536")
    ap.add_argument("--s", default="512,50")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cluster-runs", type=int, default=5)
    ap.add_argument("--budget-s", type=float, default=60.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    from cluster_cost import pair_slots, sketches
    from hulk_amd import _lib, smash
    out = open(a.out, "w") if a.out else None

    def say(line=""):
        print(line, flush=True)
        if out:
            out.write(line + "\n"); out.flush()

    L = _lib.load()
    info = L.hulk_build_info().decode()
    exp = "experiments=1" in info
    say(f"# tools/dendrogram_cost.py: default band_rows (2048); {info}")
    N_list, S_list = [int(x) for x in a.n.split(",")], [int(x) for x in a.s.split(",")]
    guess = {"jaccard": 9e12, "weightedjaccard": 5e12}      # pair-slots/s of the tile, for the budget only
    os.environ.pop("HULK_DENDRO_ROUNDS", None)

    def link_ms(m, w, metric):
        got = []
        for _ in range(a.cluster_runs):
            st = {}
            smash.cluster(m, w, 0.0, metric, stats=st)
            got.append(st["kernel_ms_link"])
        return got

    def dendro(m, w, metric, runs):
        got = []
        for _ in range(runs):
            st = {}
            smash.dendrogram(m, w, metric, stats=st)
            got.append(st)
        return got

    for s in S_list:
        rng = np.random.default_rng(s)
        base = rng.integers(0, 194481, size=s).astype(np.uint64)
        m_all, w_all = sketches(rng, max(N_list), s, base)
        say()
        say(f"== S = {s}")
        for metric in ("jaccard", "weightedjaccard"):
            say(f"  {metric}")
            smash.cluster(m_all[:256], w_all[:256], 0.0, metric); smash.dendrogram(m_all[:256], w_all[:256], metric)     # (code load)
            for n in N_list:
                work = pair_slots(n, s, metric)
                rounds_guess = 6
                if work * rounds_guess / guess[metric] > a.budget_s:
                    say(f"    N {n}: skipped: {work:.3g} pair-slots a round, above --budget-s {a.budget_s:g}")
                    continue
                m, w = m_all[:n], w_all[:n]
                before = link_ms(m, w, metric)
                got = dendro(m, w, metric, a.runs)
                first = None
                if exp:
                    os.environ["HULK_DENDRO_ROUNDS"] = "1"
                    first = dendro(m, w, metric, a.runs)
                    os.environ.pop("HULK_DENDRO_ROUNDS", None)
                after = link_ms(m, w, metric)
                med = statistics.median(before + after)
                spread = 100 * (max(before + after) - min(before + after)) / med
                best = min(got, key=lambda x: x["kernel_ms_offer"])
                per_round = best["kernel_ms_offer"] / max(best["rounds"], 1)
                say(f"    N {n}: k_cluster_link at tau = 0, ms: " + " ".join(f"{x:.3f}" for x in before) + " | " + " ".join(f"{x:.3f}" for x in after)
                    + f"  -> median {med:.3f}, spread {spread:.1f} %")
                say(f"    N {n}: dendrogram: {best['edges']} edges, {best['components']} component(s), {best['rounds']} rounds x {best['bands']} bands; "
                    f"k_dendro_offer {best['kernel_ms_offer']:.3f} ms = {per_round:.3f} ms a round = {per_round / med:.3f} x the cluster pass "
                    f"({work / (per_round * 1e-3):.4g} pair-slots/s); k_dendro_fold {best['kernel_ms_fold']:.3f} ms = "
                    f"{100 * best['kernel_ms_fold'] / (best['kernel_ms_offer'] + best['kernel_ms_fold']):.1f} % of the kernel time; "
                    f"end to end {min(x['seconds_total'] for x in got):.4f} s"
                    + ("   (all runs, offer ms: " + " ".join(f"{x['kernel_ms_offer']:.3f}" for x in got) + ")" if len(got) > 1 else ""))
                if first:
                    f = min(first, key=lambda x: x["kernel_ms_offer"])
                    say(f"    N {n}: the first round alone: k_dendro_offer {f['kernel_ms_offer']:.3f} ms = {f['kernel_ms_offer'] / med:.3f} x the cluster pass, "
                        f"k_dendro_fold {f['kernel_ms_fold']:.3f} ms; {f['edges']} edges, {f['components']} components behind it")
    L.hulk_release_caches()
    if out:
        out.close()


if __name__ == "__main__":
    main()
