#!/usr/bin/env python3
"""What a nearest-neighbour search costs (hulk_search: k_search_dist, k_search_select): profiles/search.txt.

M queries (default 1,024) against databases of P = 2,048 / 65,536 / 262,144 sketches at S = 512 and S = 50, both metrics (role row),
K = 10: kernel_ms_dist and kernel_ms_select from the library's HIP events (summed over the strips and query blocks), the distance
kernel as pair-slots per second (M x P x S over kernel_ms_dist), the call end to end (uploads of the strips from pageable host
memory included).  In the same process, before and after, `--smash-runs` runs of hulk_smash_ex (k_smash_prep + k_smash, the kernel
the rectangular one was cut from) over N = 8,192 sketches at the same S: its pair-slots per second, its run-to-run spread, and the
ratio of the two rates.  Section 2: the largest database at the first S with several scratch sizes (`--scratch-mib`): the strip size
against the distance kernel's rate.  The sketches share a base (a third of the slots agree on average), as the tests' do.

  python tools/search_cost.py [--m 1024] [--p 2048,65536,262144] [--s 512,50] [--k 10] [--smash-n 8192] [--smash-runs 5] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--p", default="2048,65536,262144")
    ap.add_argument("--s", default="512,50")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--smash-n", type=int, default=8192)
    ap.add_argument("--smash-runs", type=int, default=5)
    ap.add_argument("--scratch-mib", default="64,256,1024,4096,16384", help="section 2: the largest P at the first S with these scratch sizes")
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
    say(f"# tools/search_cost.py: M = {a.m} queries, K = {a.k}, role row, default scratch (1 GiB); {L.hulk_build_info().decode()}")
    P_list, S_list = [int(x) for x in a.p.split(",")], [int(x) for x in a.s.split(",")]
    for s in S_list:
        rng = np.random.default_rng(s)
        base = rng.integers(0, 194481, size=s).astype(np.uint64)
        qm, qw = sketches(rng, a.m, s, base)
        dm, dw = sketches(rng, max(max(P_list), a.smash_n), s, base)
        say()
        say(f"== S = {s}")

        def smash_rate(metric):
            """-> (pair-slots per second of each run, kernel_ms of each run)"""
            ms = []
            smash.distance_matrix(dm[:256], dw[:256], metric)                    # (code load)
            for _ in range(a.smash_runs):
                t = {}
                smash.distance_matrix(dm[:a.smash_n], dw[:a.smash_n], metric, timing=t)
                ms.append(t["kernel_ms"])
            return [a.smash_n * a.smash_n * s / (x * 1e-3) for x in ms], ms

        for metric in ("jaccard", "weightedjaccard"):
            rates, ms = smash_rate(metric)
            med = statistics.median(rates)
            spread = (max(rates) - min(rates)) / med
            say(f"  {metric}")
            say(f"    hulk_smash_ex N = {a.smash_n}: kernel_ms " + " ".join(f"{x:.3f}" for x in ms) +
                f"  -> median {med:.4g} pair-slots/s, run-to-run spread {100 * spread:.1f} % of it")
            say(f"    {'P':>8} {'runs':>4} {'strips':>6} {'blocks':>6} {'dist ms':>10} {'select ms':>10} {'pair-slots/s':>13} {'vs k_smash':>10} {'end to end s':>13}")
            smash.search(qm[:64], qw[:64], dm[:256], dw[:256], a.k, metric)       # (code load)
            for p in P_list:
                runs = 5 if p <= 4096 else 3 if p <= 65536 else 1
                got = []
                for _ in range(runs):
                    st = {}
                    smash.search(qm, qw, dm[:p], dw[:p], a.k, metric, stats=st)
                    got.append(st)
                best = min(got, key=lambda x: x["kernel_ms_dist"])
                rate = a.m * p * s / (best["kernel_ms_dist"] * 1e-3)
                say(f"    {p:>8} {runs:>4} {best['strips']:>6} {best['query_blocks']:>6} {best['kernel_ms_dist']:>10.3f} {best['kernel_ms_select']:>10.3f} "
                    f"{rate:>13.4g} {rate / med:>10.3f} {min(x['seconds_total'] for x in got):>13.4f}"
                    + ("   (all runs, dist ms: " + " ".join(f"{x['kernel_ms_dist']:.3f}" for x in got) + ")" if runs > 1 else ""))
            rates2, ms2 = smash_rate(metric)
            say(f"    hulk_smash_ex again: kernel_ms " + " ".join(f"{x:.3f}" for x in ms2) + f"  -> median {statistics.median(rates2):.4g} pair-slots/s")
    # section 2: the strip size.  A strip is one launch of k_search_dist per query block: its workgroups fill the chip in whole
    # rounds but for the last, and every launch is bracketed by its own events
    s, p = S_list[0], max(P_list)
    rng = np.random.default_rng(s)
    base = rng.integers(0, 194481, size=s).astype(np.uint64)
    qm, qw = sketches(rng, a.m, s, base)
    dm, dw = sketches(rng, p, s, base)
    say()
    say(f"== scratch_bytes at S = {s}, P = {p} (two runs each, the faster)")
    say(f"    {'metric':>16} {'scratch MiB':>11} {'strips':>6} {'blocks':>6} {'dist ms':>10} {'select ms':>10} {'pair-slots/s':>13} {'end to end s':>13}")
    for metric in ("jaccard", "weightedjaccard"):
        for mib in [int(x) for x in a.scratch_mib.split(",")]:
            got = []
            for _ in range(2):
                st = {}
                smash.search(qm, qw, dm, dw, a.k, metric, scratch_bytes=mib << 20, stats=st)
                got.append(st)
            best = min(got, key=lambda x: x["kernel_ms_dist"])
            say(f"    {metric:>16} {mib:>11} {best['strips']:>6} {best['query_blocks']:>6} {best['kernel_ms_dist']:>10.3f} {best['kernel_ms_select']:>10.3f} "
                f"{a.m * p * s / (best['kernel_ms_dist'] * 1e-3):>13.4g} {min(x['seconds_total'] for x in got):>13.4f}")
    L.hulk_release_caches()
    if out:
        out.close()


if __name__ == "__main__":
    main()
