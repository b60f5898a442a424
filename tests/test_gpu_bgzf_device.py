"""BGZF members inflated on the GPU (hulk_bgzf.hip): the kernel byte for byte against Python's zlib, malformed members ending in a
status that names them, and hulk_sketch_files with HULK_INGEST_DEVICE_INFLATE giving what the host readers give."""
import gzip
import hashlib
import json
import os
import pickle
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _member(text, body):
    """one BGZF member: gzip header with the BC subfield, the raw deflate `body`, CRC-32 and ISIZE of `text`"""
    total = 12 + 6 + len(body) + 8
    assert total <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\x00BC\x02\x00" + (total - 1).to_bytes(2, "little") + body
            + (zlib.crc32(text) & 0xffffffff).to_bytes(4, "little") + len(text).to_bytes(4, "little"))


def _deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """raw deflate of `text`; `flushes`: (offset, zlib flush mode) pairs cut the stream into blocks there"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    out, at = b"", 0
    for off, mode in flushes:
        out += c.compress(text[at:off]) + c.flush(mode); at = off
    return out + c.compress(text[at:]) + c.flush()


def _bgzf(text, rng, piece=65280, **kw):
    out, at = b"", 0
    while at < len(text):
        n = int(rng.integers(1, piece + 1)) if rng is not None else piece
        out += _member(text[at:at + n], _deflate(text[at:at + n], **kw)); at += n
    return out + _member(b"", _deflate(b""))


def _fastq(rng, n, L=150, crlf=False, const_q=False):
    eol = b"\r\n" if crlf else b"\n"
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    recs = []
    for i in range(n):
        s = acgt[rng.integers(0, 4, L)].tobytes()
        q = b"I" * L if const_q else (rng.integers(33, 75, L).astype(np.uint8)).tobytes()
        recs.append(b"@r%d" % i + eol + s + eol + b"+" + eol + q + eol)
    return b"".join(recs)


def _child_inflate(tmp_path, cases):
    """hulk_amd.ingest.bgzf_inflate over every case in a fresh process (under a time limit): [("ok", text) | ("err", code, msg, member)]"""
    src, dst = str(tmp_path / "cases.pkl"), str(tmp_path / "out.pkl")
    pickle.dump(cases, open(src, "wb"))
    code = ("import sys, pickle; sys.path.insert(0, %r)\nfrom hulk_amd import ingest\nfrom hulk_amd._lib import HulkError\nres = []\n"
            "for c in pickle.load(open(%r, 'rb')):\n"
            "    try: res.append(('ok', ingest.bgzf_inflate(c)))\n"
            "    except HulkError as e: res.append(('err', e.code, e.message, e.member))\n"
            "pickle.dump(res, open(%r, 'wb'))\n" % (ROOT, src, dst))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return pickle.load(open(dst, "rb"))


def test_kernel_is_byte_exact(tmp_path):
    """every kind of DEFLATE stream zlib writes: stored, fixed and dynamic blocks, several (and empty) blocks per member, 258-byte
    matches, distance-1 runs, the maximum distance, a full 64 KiB member, 1-byte members, the empty end-of-file member"""
    rng = np.random.default_rng(3)
    fq = _fastq(rng, 1500)
    rnd = rng.integers(0, 256, 32768).astype(np.uint8).tobytes()
    texts = {
        "fastq": fq,
        "runs": b"A" * 60000 + b"C" * 3000,
        "far": rnd + rnd,                                                 # 65,536 bytes, the second half 32 KiB behind the first
        "mixed": (b"ACGT" * 3000 + rnd[:2000]) * 3,
    }
    cases, want = [], []
    for name, t in texts.items():
        for kw in ({"level": 1}, {"level": 6}, {"level": 9}, {"strategy": zlib.Z_FIXED}, {"strategy": zlib.Z_HUFFMAN_ONLY},
                   {"strategy": zlib.Z_RLE}, {"flushes": ((100, zlib.Z_FULL_FLUSH), (5000, zlib.Z_SYNC_FLUSH), (5000, zlib.Z_SYNC_FLUSH),
                                                         (20000, zlib.Z_FULL_FLUSH))}):
            bodies = [(t[a:a + 65536], _deflate(t[a:a + 65536], **kw)) for a in range(0, len(t), 65536)]
            if any(len(b) > 65536 - 26 for _, b in bodies):                   # (Huffman only / fixed codes on random bytes: too big)
                continue
            cases.append(b"".join(_member(x, b) for x, b in bodies)); want.append(t)
        stored = t[:60000]
        cases.append(_member(stored, _deflate(stored, level=0))); want.append(stored)
    one = b"".join(_member(bytes([c]), _deflate(bytes([c]), level=lv)) for c, lv in zip(b"ACGT\n@+", (0, 1, 6, 9, 0, 1, 6)))
    cases.append(one); want.append(b"ACGT\n@+")
    cases.append(_member(b"", _deflate(b""))); want.append(b"")
    cases.append(_bgzf(fq * 4, rng)); want.append(fq * 4)
    cases.append(b""); want.append(b"")
    res = _child_inflate(tmp_path, cases)
    for i, (r, w) in enumerate(zip(res, want)):
        assert r[0] == "ok", (i, r)
        assert r[1] == w, i
        assert r[1] == (gzip.decompress(cases[i]) if cases[i] else b"")


class _Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, n):
        self.v |= value << self.n; self.n += n

    def huff(self, code, n):                   # Huffman codes go MSB first
        self.put(int(format(code, "0%db" % n)[::-1], 2), n)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def test_kernel_malformed_members_end_in_a_status(tmp_path):
    """a flipped payload bit, a wrong CRC or ISIZE, a cut payload, an over-subscribed code, a distance before the member's start:
    an error naming the member (the members in front are fine); the process survives and the next call works"""
    rng = np.random.default_rng(5)
    fq = _fastq(rng, 800)
    good = [_member(fq[a:a + 30000], _deflate(fq[a:a + 30000])) for a in range(0, len(fq), 30000)]
    k = 2
    body = _deflate(fq[k * 30000:(k + 1) * 30000])
    text = fq[k * 30000:(k + 1) * 30000]

    def with_k(m):
        return b"".join(good[:k]) + m + b"".join(good[k + 1:])
    cases = []
    for bit in (5, 800, 4000, len(body) * 8 - 20):
        b = bytearray(body); b[bit // 8] ^= 1 << (bit % 8)
        cases.append(with_k(_member(text, bytes(b))))
    m = bytearray(_member(text, body)); m[-8] ^= 0x40; cases.append(with_k(bytes(m)))        # CRC
    m = bytearray(_member(text, body)); m[-4] ^= 0x01; cases.append(with_k(bytes(m)))        # ISIZE one off
    m = bytearray(_member(text, body)); m[-3] ^= 0x01; cases.append(with_k(bytes(m)))        # ISIZE 256 off
    cases.append(with_k(_member(text, body[:len(body) // 2])))                               # payload cut (BSIZE agrees)
    cases.append(with_k(_member(text, body + b"\0\0")))                                      # bytes behind the deflate end
    w = _Bits(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(0, 4)             # dynamic: 257 + 1 codes, 4 code-length codes
    for ln in (1, 1, 1, 0):                                                                  # three 1-bit codes: over-subscribed
        w.put(ln, 3)
    cases.append(with_k(_member(b"xyz", w.bytes() + b"\0" * 8)))
    w = _Bits(); w.put(1, 1); w.put(1, 2)                                                    # fixed: 'A', then length 3 at distance 5
    w.huff(0x30 + 65, 8); w.huff(1, 7); w.huff(4, 5); w.put(0, 1); w.huff(0, 7)
    cases.append(with_k(_member(b"AAAA", w.bytes())))
    w = _Bits(); w.put(1, 1); w.put(3, 2)                                                    # block type 3
    cases.append(with_k(_member(b"", w.bytes())))
    cases.append(b"".join(good))                                                             # and the process is still fine
    res = _child_inflate(tmp_path, cases)
    for i, r in enumerate(res[:-1]):
        assert r[0] == "err", (i, r)
        assert r[3] == k and ("member %d " % k) in r[2], (i, r)
    assert res[-1] == ("ok", fq)
    # framing: a member that is not whole names itself too
    res = _child_inflate(tmp_path, [b"".join(good)[:-5], b"".join(good) + b"junk"])
    assert res[0][0] == "err" and res[0][3] == len(good) - 1
    assert res[1][0] == "err" and res[1][3] == len(good)


def _run(paths, flags, fasta=False, block=131072, k=15, w=9, S=64, interval=3000):
    """(stats, sketch, counters) of one hulk_sketch_files run, or ("error", code, message)"""
    import hulk_amd
    from hulk_amd._lib import HulkError
    g = hulk_amd.GpuSketcher(k, w, S, interval=interval)
    try:
        st = g.sketch_files(paths, fasta=fasta, opts={"flags": flags, "block_bytes": block})
        g.finish()
        return (st["n_seqs"], st["total_len"], st["n_lines"], st["bytes_in"]), g.sketch(), g.counters()
    except HulkError as e:
        return ("error", e.code, e.message)
    finally:
        g.close()


def _same(a, b):
    if a[0] == "error" or b[0] == "error":
        return a == b
    return a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1])


def _dev_flags():
    from hulk_amd import _lib
    return _lib.HULK_INGEST_DEVICE_INFLATE | _lib.HULK_INGEST_TRACE


def test_sketch_path_equals_the_host_path(tmp_path, capfd):
    """FASTQ over many 128 KiB blocks (records straddle members and blocks, CRLF, no final newline), --fasta with contigs over
    many members, and a list mixing BGZF, plain and one-member .gz: the same stats, sketch and counters with the flag as without"""
    rng = np.random.default_rng(7)
    fq = _fastq(rng, 4000, crlf=False) + _fastq(rng, 500, crlf=True)
    p1 = str(tmp_path / "a.fq.gz"); open(p1, "wb").write(_bgzf(fq.rstrip(b"\r\n"), rng))
    r0, r1 = _run([p1], 0), _run([p1], _dev_flags())
    assert r0[0] != "error" and r0[0][0] == 4500 and _same(r0, r1)
    err = capfd.readouterr().err
    assert "members inflated on the GPU" in err and "handed over" not in err
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    fa = b"".join(b">c%d\n" % i + b"\n".join(acgt[rng.integers(0, 4, 70)].tobytes() for _ in range(int(rng.integers(50, 3000)))) + b"\n"
                  for i in range(60))
    p2 = str(tmp_path / "c.fa.gz"); open(p2, "wb").write(_bgzf(fa, rng, piece=20000))
    r0, r1 = _run([p2], 0, fasta=True, k=11, w=5), _run([p2], _dev_flags(), fasta=True, k=11, w=5)
    assert r0[0] != "error" and r0[0][0] == 60 and _same(r0, r1)
    assert "members inflated on the GPU" in capfd.readouterr().err
    more = _fastq(rng, 700)
    p3 = str(tmp_path / "b.fq"); open(p3, "wb").write(more[:-1])
    p4 = str(tmp_path / "d.fq.gz"); open(p4, "wb").write(gzip.compress(_fastq(rng, 900), 6))
    r0, r1 = _run([p1, p3, p4, p1], 0), _run([p1, p3, p4, p1], _dev_flags())
    assert r0[0] != "error" and r0[0][0] == 4500 * 2 + 700 + 900 and _same(r0, r1)
    assert capfd.readouterr().err.count("members inflated on the GPU") == 2


def test_failures_are_those_of_the_host_path(tmp_path, capfd):
    """an ordinary member and junk between BGZF members, a lying BSIZE, a bad CRC in member 4, a cut file, the EOF member alone:
    the same reads or the same message as the host readers, the hand-over in the trace"""
    rng = np.random.default_rng(11)
    blob = _fastq(rng, 12000)
    cut1, cut2 = blob.index(b"\n@r4000\n") + 1, blob.index(b"\n@r8000\n") + 1
    good = _bgzf(blob, rng)
    hdr = [i for i in range(len(good) - 18) if good[i:i + 4] == b"\x1f\x8b\x08\x04" and good[i + 12:i + 16] == b"BC\x02\x00"]
    files = {}
    files["mixed"] = _bgzf(blob[:cut1], rng)[:-28] + gzip.compress(blob[cut1:cut2], 6) + _bgzf(blob[cut2:], rng) + b"\0\0not gzip"
    lying = bytearray(good); at = hdr[2] + 16
    lying[at:at + 2] = (int.from_bytes(good[at:at + 2], "little") + 7).to_bytes(2, "little")
    files["lying"] = bytes(lying)
    bad = bytearray(good); bad[hdr[5] - 6] ^= 0x20
    files["crc"] = bytes(bad)
    files["cut"] = good[:hdr[len(hdr) // 2] + 300]
    files["empty"] = _member(b"", _deflate(b""))
    for name, data in files.items():
        p = str(tmp_path / (name + ".fq.gz")); open(p, "wb").write(data)
        r0, r1 = _run([p], 0), _run([p], _dev_flags())
        assert _same(r0, r1), (name, r0[0], r1[0])
        err = capfd.readouterr().err
        assert "BGZF device reader" in err, name
        if name in ("mixed", "lying", "crc", "cut"):
            assert "handed over to the sequential reader at byte" in err, name
    assert _run([str(tmp_path / "crc.fq.gz")], _dev_flags()) == ("error", -35, "gzip: invalid checksum")
    assert _run([str(tmp_path / "cut.fq.gz")], _dev_flags()) == ("error", -35, "unexpected EOF")
    assert _run([str(tmp_path / "mixed.fq.gz")], _dev_flags())[0][0] == 12000


def test_release_caches_and_the_environment_switch(tmp_path):
    """hulk_release_caches() between runs gives the same result; HULK_GZ_DEVICE=1 in a fresh process behaves like the flag"""
    from hulk_amd import _lib
    rng = np.random.default_rng(13)
    fq = _fastq(rng, 3000)
    p = str(tmp_path / "a.fq.gz"); open(p, "wb").write(_bgzf(fq, rng))
    a = _run([p], _lib.HULK_INGEST_DEVICE_INFLATE)
    assert _lib.load().hulk_release_caches() == 0
    b = _run([p], _lib.HULK_INGEST_DEVICE_INFLATE)
    c = _run([p], 0)
    assert _same(a, b) and _same(a, c)
    code = ("import sys, hashlib; sys.path.insert(0, %r)\nimport hulk_amd\ng = hulk_amd.GpuSketcher(15, 9, 64, interval=3000)\n"
            "st = g.sketch_files([%r], opts={'block_bytes': 131072}); g.finish()\n"
            "print(st['n_seqs'], hashlib.md5(g.sketch()[0].astype('<u8').tobytes()).hexdigest())\n" % (ROOT, p))
    env = dict(os.environ, HULK_GZ_DEVICE="1", HULK_INGEST_TRACE="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "members inflated on the GPU" in r.stderr
    assert r.stdout.split() == [str(a[0][0]), hashlib.md5(a[1][0].astype("<u8").tobytes()).hexdigest()]


def test_fuzz_slice(tmp_path):
    """tools/fuzz_bgzf_device.py --cases 200: device inflate against the host readers, 0 mismatches"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_bgzf_device.py"), "--cases", "200", "--seed", "1",
                        "--dir", str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["cases"] == 200 and res["mismatches"] == 0 and res["device_members"] > 0
