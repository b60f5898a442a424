#!/usr/bin/env python3
"""What a search through the banded index costs against hulk_search (hulk_index_search: k_index_keys, k_index_probe, k_index_verify,
k_index_select): profiles/index.txt.

M queries (default 1,024) and a single query (the service case) against N = 262,144 sketches at S = 512, jaccard, K = 10, at the build
thresholds D = 0.05, 0.1 and 0.2, the search limit equal to D.  Two collections:
  families   3/4 of the collection in families of 64 over a family base, each member with its own share of 0 - 30 % replaced slots;
             the rest unrelated sketches.  The queries are further members of random families
  random     search_cost.py's set: every sketch keeps 20 - 80 % of ONE base — any two sketches share many slots: the filter's worst case
Per leg: the build (seconds, device bytes, bands), then index search and hulk_search on the same host arrays in alternating runs:
medians and spread ((max - min) / median) of the end-to-end seconds, the index's candidates per query, the kernel milliseconds per phase
(medians) and the ratio hulk_search / index.  The two results are compared byte for byte once per leg.

  python tools/index_cost.py [--n 262144] [--m 1024] [--s 512] [--d 0.05,0.1,0.2] [--sets families,random] [--runs 5] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def family_set(rng, n, m, s):
    import numpy as np
    fam, per = max(n * 3 // 4 // 64, 1), 64
    bases = rng.integers(0, 1 << 40, size=(fam, s)).astype(np.uint64)

    def members(of):
        share = rng.random((len(of), 1)) * 0.3
        return np.where(rng.random((len(of), s)) < share, rng.integers(0, 1 << 40, size=(len(of), s)).astype(np.uint64), bases[of])
    db = np.vstack([members(np.repeat(np.arange(fam), per)), rng.integers(0, 1 << 40, size=(n - fam * per, s)).astype(np.uint64)])
    db = db[rng.permutation(n)]
    return np.ascontiguousarray(members(rng.integers(0, fam, size=m))), np.ascontiguousarray(db)


def random_set(rng, n, m, s):
    import numpy as np
    base = rng.integers(0, 194481, size=s).astype(np.uint64)

    def sketches(c):
        keep = rng.random((c, 1)) * 0.6 + 0.2 > rng.random((c, s))
        return np.ascontiguousarray(np.where(keep, base[None, :], rng.integers(0, 194481, size=(c, s)).astype(np.uint64)))
    return sketches(m), sketches(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--s", type=int, default=512)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--d", default="0.05,0.1,0.2")
    ap.add_argument("--sets", default="families,random")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    from hulk_amd import _lib, smash
    out = open(a.out, "w") if a.out else None

    def say(line=""):
        print(line, flush=True)
        if out:
            out.write(line + "\n"); out.flush()

    def spread(v):
        return 100.0 * (max(v) - min(v)) / statistics.median(v)

    L = _lib.load()
    say(f"# tools/index_cost.py: N = {a.n}, S = {a.s}, K = {a.k}, jaccard, search limit = build threshold, default scratch, {a.runs} alternating runs; "
        f"{L.hulk_build_info().decode()}")
    for name in a.sets.split(","):
        rng = np.random.default_rng(len(name))
        qm, dm = (family_set if name == "families" else random_set)(rng, a.n, a.m, a.s)
        qw, dw = np.ones(qm.shape), np.ones(dm.shape)
        say()
        say(f"== {name}")
        for d in [float(x) for x in a.d.split(",")]:
            t0 = time.perf_counter()
            ix = smash.Index.build(dm, d)
            t_build = time.perf_counter() - t0
            info = ix.info
            say(f"  D = {d}: {info['bands']} bands of {a.s // info['bands']} - {-(-a.s // info['bands'])} slots, build {t_build:.3f} s, "
                f"device bytes {info['device_bytes']} ({info['device_bytes'] / a.n:.0f} a sketch)")
            say("      M  cand / query  hits / query    keys ms   probe ms  verify ms  select ms   index s (median, spread)  search s (median, spread)"
                "  dist ms  select ms  search / index")
            for m in (a.m, 1):
                ti, ts, st_i, st_s = [], [], [], []
                smash.search(qm[:m], qw[:m], dm, dw, a.k, "jaccard", max_distance=d)        # (warm-up of both)
                ix.search(qm[:m], a.k)
                for _ in range(a.runs):
                    st = {}
                    t0 = time.perf_counter(); got = ix.search(qm[:m], a.k, stats=st); ti.append(time.perf_counter() - t0); st_i.append(st)
                    st = {}
                    t0 = time.perf_counter(); ref = smash.search(qm[:m], qw[:m], dm, dw, a.k, "jaccard", max_distance=d, stats=st)
                    ts.append(time.perf_counter() - t0); st_s.append(st)
                same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, ref))
                med = lambda rows, key: statistics.median(r[key] for r in rows)          # noqa: E731
                say(f"  {m:5d}  {st_i[0]['candidates'] / m:12.1f}  {st_i[0]['within'] / m:12.1f}  {med(st_i, 'kernel_ms_keys'):9.3f}  "
                    f"{med(st_i, 'kernel_ms_probe'):9.3f}  {med(st_i, 'kernel_ms_verify'):9.3f}  {med(st_i, 'kernel_ms_select'):9.3f}  "
                    f"{statistics.median(ti):12.5f}  {spread(ti):6.1f} %  {statistics.median(ts):13.5f}  {spread(ts):6.1f} %  "
                    f"{med(st_s, 'kernel_ms_dist'):7.3f}  {med(st_s, 'kernel_ms_select'):9.3f}  {statistics.median(ts) / statistics.median(ti):14.2f}"
                    f"{'' if same else '   RESULTS DIFFER'}")
            ix.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
