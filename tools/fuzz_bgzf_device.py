#!/usr/bin/env python3
"""Device BGZF inflate (HULK_INGEST_DEVICE_INFLATE) against the host readers: random FASTQ / FASTA texts cut into members of
random sizes, each deflated with a random zlib level / strategy / flush points; ordinary gzip members mixed in; corruption of a
payload bit, a CRC, an ISIZE, a BSIZE; truncation and trailing bytes.  Every case is sketched with and without the flag (same
process, same parameters): stats, sketch, counters or error message must agree.  --crafted: the members are written by
tests/deflate_craft.py instead of zlib — FASTQ built from tokens, small blocks with random code shapes (codes of up to 15 bits,
lone and absent distance codes, 7-bit code-length codes), the shapes of other encoders; the corruptions stay the same.
usage: fuzz_bgzf_device.py [--cases N] [--seed S] [--dir D] [--crafted]   (last stdout line: a JSON summary)"""
import argparse, gzip, json, os, re, sys, tempfile, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import hulk_amd
from hulk_amd import _lib
from hulk_amd._lib import HulkError

STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED)


def member(text, body):
    total = 12 + 6 + len(body) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\x00BC\x02\x00" + (total - 1).to_bytes(2, "little") + body
            + (zlib.crc32(text) & 0xffffffff).to_bytes(4, "little") + len(text).to_bytes(4, "little"))


def deflate(rng, text):
    c = zlib.compressobj(int(rng.integers(0, 10)), zlib.DEFLATED, -15, 8, STRATEGIES[int(rng.integers(0, len(STRATEGIES)))])
    out, at = b"", 0
    for off in sorted(int(x) for x in rng.integers(0, len(text) + 1, int(rng.integers(0, 4)))):
        out += c.compress(text[at:off]) + c.flush(zlib.Z_FULL_FLUSH if rng.random() < 0.5 else zlib.Z_SYNC_FLUSH); at = off
    return out + c.compress(text[at:]) + c.flush()


def text_of(rng):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    if rng.random() < 0.75:
        eol = b"\r\n" if rng.random() < 0.2 else b"\n"
        out = []
        for i in range(int(rng.integers(1, 1500))):
            L = int(rng.integers(20, 300))
            q = b"I" * L if rng.random() < 0.3 else rng.integers(33, 75, L).astype(np.uint8).tobytes()
            out.append(b"@r%d" % i + eol + acgt[rng.integers(0, 4, L)].tobytes() + eol + b"+" + eol + q + eol)
        t = b"".join(out)
    else:
        t = b"".join(b">c%d\n" % i + b"\n".join(acgt[rng.integers(0, 4, 60)].tobytes() for _ in range(int(rng.integers(1, 400)))) + b"\n"
                     for i in range(int(rng.integers(1, 40))))
    if rng.random() < 0.2:
        t = t.rstrip(b"\r\n")
    return t, t.startswith(b">")


def crafted(rng):
    """(members, text) from the test encoder: a FASTQ of 1 KB - 400 KB in members of random sizes"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import deflate_craft
    hi = int(rng.choice([2000, 20000, 65280]))
    members, _, _ = deflate_craft.fastq_bgzf_members(int(rng.integers(0, 2 ** 31)), int(rng.choice([1000, 30000, 150000, 400000])), lo=300, hi=hi)
    if rng.random() >= 0.8:
        members.pop()                                                                        # (no end-of-file member)
    return members


def container(rng, text, members=None):
    out, at = members or [], 0
    big = rng.random() < 0.5
    while members is None and at < len(text):
        n = 65280 if big and rng.random() < 0.7 else int(rng.integers(1, 65281))
        piece = text[at:at + n]; at += n
        if rng.random() < 0.05:
            out.append(gzip.compress(piece, 6))                                              # an ordinary gzip member
        else:
            body = deflate(rng, piece)
            if 12 + 6 + len(body) + 8 > 65536:                                                # (incompressible: stored)
                c = zlib.compressobj(0, zlib.DEFLATED, -15); body = c.compress(piece) + c.flush()
            out.append(member(piece, body))
    if members is None and rng.random() < 0.8:
        out.append(member(b"", deflate(rng, b"")))
    data = bytearray(b"".join(out))
    kind = "clean"
    if rng.random() < 0.35 and len(out) > 0:
        kind = ["payload", "crc", "isize", "bsize", "truncate", "trailing"][int(rng.integers(0, 6))]
        k = int(rng.integers(0, len(out))); start = sum(len(m) for m in out[:k]); m = out[k]
        if kind == "payload" and len(m) > 28:
            data[start + 18 + int(rng.integers(0, len(m) - 26))] ^= 1 << int(rng.integers(0, 8))
        elif kind == "crc":
            data[start + len(m) - 8 + int(rng.integers(0, 4))] ^= 1 << int(rng.integers(0, 8))
        elif kind == "isize":
            data[start + len(m) - 4 + int(rng.integers(0, 3))] ^= 1 << int(rng.integers(0, 8))
        elif kind == "bsize":
            data[start + 16] ^= 1 << int(rng.integers(0, 8))
        elif kind == "truncate":
            del data[int(rng.integers(0, len(data))):]
        else:
            data += rng.integers(0, 256, int(rng.integers(1, 40))).astype(np.uint8).tobytes()
    return bytes(data), kind


def run(paths, fasta, flags, block):
    g = hulk_amd.GpuSketcher(11 if fasta else 15, 5 if fasta else 9, 32, interval=0 if fasta else 2000)
    try:
        st = g.sketch_files(paths, fasta=fasta, opts={"flags": flags, "block_bytes": block})
        g.finish()
        m, w = g.sketch()
        return ("ok", st["n_seqs"], st["total_len"], st["n_lines"], st["bytes_in"], m.tobytes(), w.tobytes(), tuple(g.counters().items()))
    except HulkError as e:
        return ("error", e.code, e.message)
    finally:
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--crafted", action="store_true")
    a = ap.parse_args()
    d = tempfile.mkdtemp(dir=a.dir)
    log = os.path.join(d, "trace.txt")
    rng = np.random.default_rng(a.seed)
    mismatches, members, kinds = 0, 0, {}
    for case in range(a.cases):
        if a.crafted:
            fasta = False
            data, kind = container(rng, None, crafted(rng))
        else:
            text, fasta = text_of(rng)
            data, kind = container(rng, text)
        kinds[kind] = kinds.get(kind, 0) + 1
        p = os.path.join(d, "c%d.%s.gz" % (case, "fa" if fasta else "fq"))
        open(p, "wb").write(data)
        paths = [p]
        if rng.random() < 0.2:                                           # a list: a plain file behind it
            q = os.path.join(d, "c%d.txt" % case); open(q, "wb").write(text_of(rng)[0] if not fasta else b">x\nACGTACGTACGTAC\n"); paths.append(q)
        block = int(rng.choice([131072, 262144, 1 << 20]))
        host = run(paths, fasta, 0, block)
        fd = os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC); saved = os.dup(2); os.dup2(fd, 2); os.close(fd)
        try:
            dev = run(paths, fasta, _lib.HULK_INGEST_DEVICE_INFLATE | _lib.HULK_INGEST_TRACE, block)
        finally:
            os.dup2(saved, 2); os.close(saved)
        members += sum(int(x) for x in re.findall(r"BGZF device reader, (\d+) members", open(log).read()))
        if host != dev:
            mismatches += 1
            print("MISMATCH case %d (%s, fasta=%s): host %r | device %r" % (case, kind, fasta, host[:5], dev[:5]), flush=True)
        os.remove(p)
    print(json.dumps({"cases": a.cases, "mismatches": mismatches, "device_members": members, "kinds": kinds, "seed": a.seed, "crafted": a.crafted}))
    return 1 if mismatches else 0


if __name__ == "__main__":
    sys.exit(main())
