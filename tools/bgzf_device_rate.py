#!/usr/bin/env python3
"""bgzip'd FASTQ file -> sketch (C2 parameters): members inflated on the GPU (HULK_INGEST_DEVICE_INFLATE) against the host's BGZF
reader (GzBgzf, 16 threads), on the same file in the same process, runs alternating; the plain file through the device parser
for scale.  Prints every run, then median and spread per path, and the sketch md5 of each path (they must be one).
usage: bgzf_device_rate.py [reads (8000000)] [runs per path (5)] [quals: random|const]"""
import hashlib, os, shutil, statistics, sys, tempfile, time, zlib
import multiprocessing
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def bgzf_piece(piece):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(piece) + c.flush()
    total = 12 + 6 + len(body) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\x00BC\x02\x00" + (total - 1).to_bytes(2, "little") + body
            + (zlib.crc32(piece) & 0xffffffff).to_bytes(4, "little") + len(piece).to_bytes(4, "little"))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8_000_000
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    quals = sys.argv[3] if len(sys.argv) > 3 else "random"
    import hulk_amd
    from hulk_amd import _lib, synth
    L = 150
    d = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    plain, gz = os.path.join(d, "r.fq"), os.path.join(d, "r.fq.gz")
    rng = np.random.default_rng(1)
    with open(plain, "wb") as fh:
        for first in range(0, n, 500_000):
            m = min(500_000, n - first)
            bases = synth.reads_numpy(first, m, L)[0][:m * L].reshape(m, L)
            rec = np.empty((m, 8 + 1 + L + 1 + 2 + L + 1), dtype=np.uint8)
            ids = np.char.zfill(np.arange(first, first + m).astype("U7"), 7)
            rec[:, 0] = ord("@"); rec[:, 1:8] = np.frombuffer("".join(ids).encode(), dtype=np.uint8).reshape(m, 7); rec[:, 8] = ord("\n")
            rec[:, 9:9 + L] = bases; rec[:, 9 + L] = ord("\n"); rec[:, 10 + L] = ord("+"); rec[:, 11 + L] = ord("\n")
            rec[:, 12 + L:12 + 2 * L] = ord("I") if quals == "const" else rng.integers(33, 75, (m, L)).astype(np.uint8)
            rec[:, 12 + 2 * L] = ord("\n")
            fh.write(rec.tobytes())
    text = open(plain, "rb").read()
    with multiprocessing.get_context("spawn").Pool(16) as pool, open(gz, "wb") as fh:
        for m in pool.imap(bgzf_piece, (text[a:a + 65280] for a in range(0, len(text), 65280)), chunksize=64):
            fh.write(m)
        fh.write(bgzf_piece(b""))
    del text
    size, csize = os.path.getsize(plain), os.path.getsize(gz)
    print("file: %d reads, %s qualities, %.1f MB of text, %.1f MB bgzip'd (ratio %.2f)" % (n, quals, size / 1e6, csize / 1e6, size / csize), flush=True)
    legs = (("device", gz, _lib.HULK_INGEST_DEVICE_INFLATE), ("host", gz, 0), ("plain", plain, 0))
    times = {k: [] for k, _, _ in legs}
    md5 = {k: set() for k, _, _ in legs}
    for r in range(runs + 1):                                              # run 0 of each leg: warm-up (allocations), not counted
        for name, path, flags in legs:
            sk = hulk_amd.GpuSketcher(21, 9, 512, interval=100_000)
            t0 = time.perf_counter(); sk.sketch_files([path], opts={"flags": flags} if flags else None); sk.finish(); dt = time.perf_counter() - t0
            md5[name].add(hashlib.md5(sk.sketch()[0].astype("<u8").tobytes()).hexdigest()[:8])
            sk.close()
            if r:
                times[name].append(dt)
            print("run %d %-6s: %.1f ms, %.3g reads/s, %.2f GB/s of text" % (r, name, dt * 1e3, n / dt, size / dt / 1e9), flush=True)
    for name, _, _ in legs:
        t = sorted(times[name])
        med = statistics.median(t)
        print("%-6s median %.1f ms (%.3g reads/s, %.2f GB/s of text), min %.1f max %.1f ms over %d runs | sketch_md5 %s"
              % (name, med * 1e3, n / med, size / med / 1e9, t[0] * 1e3, t[-1] * 1e3, len(t), ",".join(sorted(md5[name]))), flush=True)
    print("device / host BGZF: %.2fx; device / plain: %.2fx" % (statistics.median(times["host"]) / statistics.median(times["device"]),
                                                                statistics.median(times["plain"]) / statistics.median(times["device"])))
    shutil.rmtree(d)


if __name__ == "__main__":
    main()
