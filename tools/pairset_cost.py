#!/usr/bin/env python3
"""The five pair-tile jobs of one library build in one process: profiles/pairset.txt.

8,192 sketches (tools/cluster_cost.py's sets) at S = 512 and S = 50, jaccard and weightedjaccard, and the first 2,048 of them
as bottom-k lists: k_search_dist (a --self search; weighted also role column against the set itself), k_cluster_link at
tau = 0, k_links_count and k_links_fill at the 1 % quantile of the distances (jaccard and bottomk with `upper`), k_dendro_offer summed over the rounds — each from the library's HIP events, a warm-up
call, then three runs and their median.  To compare two builds run the processes alternately, HULK_LIB=<path> naming the other
library (hulk_amd/_lib.py), and hold the medians of one against the spread of the other's.

  python tools/pairset_cost.py TAG
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    from hulk_amd import smash
    tag, n = sys.argv[1], 8192
    for s in (512, 50):
        rng = np.random.default_rng(s)
        base = rng.integers(0, 194481, size=s).astype(np.uint64)
        keep = rng.random((n, 1)) * 0.6 + 0.2 > rng.random((n, s))
        m = np.ascontiguousarray(np.where(keep, base[None, :], rng.integers(0, 194481, size=(n, s)).astype(np.uint64)))
        w = -rng.gamma(2.0, 1e-3, size=(n, s))
        D = smash.distance_matrix(m[:1024], w[:1024], "jaccard")
        off = D[~np.eye(1024, dtype=bool)]
        q1 = float(np.quantile(off[~np.isnan(off)], 0.01))
        for metric in ("jaccard", "weightedjaccard", "bottomk"):
            upper = metric != "weightedjaccard"
            if metric == "bottomk":                              # the merge tile is some 25 x the slot loop: a quarter of the set
                m, w = np.ascontiguousarray(m[:2048]), None
                D = smash.distance_matrix(m[:1024], None, metric)
                off = D[~np.eye(1024, dtype=bool)]
                q1 = float(np.quantile(off, 0.01))
            cells = {
                "search_row": lambda st: (smash.search(m, w, None, None, 10, metric, self_search=True, stats=st), st["kernel_ms_dist"])[1],
                "cluster_link": lambda st: (smash.cluster(m, w, 0.0, metric, stats=st), st["kernel_ms_link"])[1],
                "links_count": lambda st: (smash.links(m, w, q1, metric, upper=upper, stats=st), st["kernel_ms_count"])[1],
                "links_fill": lambda st: (smash.links(m, w, q1, metric, upper=upper, stats=st), st["kernel_ms_fill"])[1],
                "dendro_offer": lambda st: (smash.dendrogram(m, w, metric, stats=st), st["kernel_ms_offer"])[1],
            }
            if metric == "weightedjaccard":
                cells["search_col"] = lambda st: (smash.search(m, w, m, w, 10, metric, role="column", stats=st), st["kernel_ms_dist"])[1]
            for name, f in cells.items():
                f({})                                            # (code load)
                got = [f({}) for _ in range(3)]
                print(f"{tag} S={s} {metric} {name} ms " + " ".join(f"{x:.3f}" for x in got) + f" median {statistics.median(got):.3f}", flush=True)


if __name__ == "__main__":
    main()
