#!/usr/bin/env python3
"""What the sparse link list costs (hulk_links: k_links_count, k_links_fill): profiles/links.txt.

N sketches (default 8,192 and 65,536) at S = 512 and S = 50, jaccard and weightedjaccard, on one set per S, in one process:
  1. the count pass against the link kernel, where nothing links (tau = 0): kernel_ms_count of hulk_links and kernel_ms_link of
     hulk_cluster from the libraries' HIP events summed over the bands, `--runs` runs of each, ALTERNATING, the medians, the spread of
     either and the ratio.  jaccard with upper=True computes the tiles k_cluster_link computes (the staircase on and above the
     diagonal); weightedjaccard computes the full square in both.  jaccard without upper (the full square) is given beside it.
  2. the whole call (seconds_total: upload, preparation, both passes, the copies) at thresholds that give about 1, 16 and 256 edges
     per row — quantiles of the distances of the first 1,024 sketches; the edges per row that came out are printed — and with every
     pair linked (tau = 1): count ms, fill ms, seconds, and the bytes of edges (12 an edge) delivered to the host per second of the
     whole call.  `--runs-call` runs each, the median and the spread.
A case whose edges alone would take more than `--max-edge-gb` of host memory is skipped and said so.

  python tools/links_cost.py [--n 8192,65536] [--s 512,50] [--runs 5] [--runs-call 3] [--max-edge-gb 8] [--out FILE]
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


def spread(xs):
    return 100 * (max(xs) - min(xs)) / statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="8192,65536")
    ap.add_argument("--s", default="512,50")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--runs-call", type=int, default=3)
    ap.add_argument("--max-edge-gb", type=float, default=8.0)
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
    say(f"# tools/links_cost.py: default band_rows (2048); {L.hulk_build_info().decode()}")
    N_list, S_list = [int(x) for x in a.n.split(",")], [int(x) for x in a.s.split(",")]
    for s in S_list:
        rng = np.random.default_rng(s)
        base = rng.integers(0, 194481, size=s).astype(np.uint64)
        m_all, w_all = sketches(rng, max(N_list), s, base)
        say()
        say(f"== S = {s}")
        for metric in ("jaccard", "weightedjaccard"):
            say(f"  {metric}")
            smash.cluster(m_all[:256], w_all[:256], 0.5, metric)                 # (code load)
            smash.links(m_all[:256], w_all[:256], 0.5, metric)
            smash.links(m_all[:256], w_all[:256], 0.5, metric, upper=True)
            D = smash.distance_matrix(m_all[:1024], w_all[:1024], metric)
            off = D[~np.eye(len(D), dtype=bool)]
            off = off[~np.isnan(off)]
            say("    1. nothing links (tau = 0): k_links_count against k_cluster_link, ms summed over the bands")
            say(f"    {'N':>7} {'form':>12} {'runs':>4} {'link ms (median, spread)':>26} {'count ms (median, spread)':>26} {'count / link':>12}")
            for n in N_list:
                m, w = m_all[:n], w_all[:n]
                forms = (("upper", True), ("full square", False)) if metric == "jaccard" else (("full square", False),)
                for form, upper in forms:
                    link, count, edges = [], [], 0
                    for _ in range(a.runs):                                      # alternating
                        st = {}
                        smash.cluster(m, w, 0.0, metric, stats=st)
                        link.append(st["kernel_ms_link"]); edges += st["links"]
                        st = {}
                        smash.links(m, w, 0.0, metric, upper=upper, stats=st)
                        count.append(st["kernel_ms_count"]); edges += st["edges"]
                    if edges:
                        say("    (the set holds identical pairs: the next line is NOT a run without links)")
                    ml, mc = statistics.median(link), statistics.median(count)
                    say(f"    {n:>7} {form:>12} {a.runs:>4} {ml:>16.3f} {spread(link):>8.1f} % {mc:>16.3f} {spread(count):>8.1f} % {mc / ml:>12.3f}")
            say("    2. the whole call")
            say(f"    {'N':>7} {'tau':>10} {'edges':>12} {'per row':>9} {'max degree':>10} {'count ms':>10} {'fill ms':>10} {'seconds (median, spread)':>26} {'edge MB/s':>10}")
            for n in N_list:
                m, w = m_all[:n], w_all[:n]
                for want in (1, 16, 256, None):
                    tau = 1.0 if want is None else float(np.quantile(off, min(1.0, want / n), method="lower"))
                    if want is None and n * (n - 1) * 12 > a.max_edge_gb * 2 ** 30:
                        say(f"    {n:>7} {'1':>10} skipped: {n * (n - 1)} edges are {n * (n - 1) * 12 / 2 ** 30:.1f} GiB on the host, above --max-edge-gb {a.max_edge_gb:g}")
                        continue
                    got = []
                    try:
                        for _ in range(a.runs_call):
                            st = {}
                            smash.links(m, w, tau, metric, max_edges=int(a.max_edge_gb * 2 ** 30 / 12), stats=st)
                            got.append(st)
                    except _lib.HulkError as e:
                        say(f"    {n:>7} {tau:>10.4f} skipped: {e.message}")
                        continue
                    secs = [x["seconds_total"] for x in got]
                    mid = sorted(got, key=lambda x: x["seconds_total"])[len(got) // 2]
                    say(f"    {n:>7} {tau:>10.4f} {mid['edges']:>12} {mid['edges'] / n:>9.1f} {mid['max_degree']:>10} {mid['kernel_ms_count']:>10.3f} {mid['kernel_ms_fill']:>10.3f} "
                        f"{statistics.median(secs):>16.4f} {spread(secs):>8.1f} % {12e-6 * mid['edges'] / statistics.median(secs):>10.1f}")
    L.hulk_release_caches()
    if out:
        out.close()


if __name__ == "__main__":
    main()
