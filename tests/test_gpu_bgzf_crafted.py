"""k_bgzf_inflate (hulk_bgzf.hip) on DEFLATE streams zlib's encoder never writes: the corpus of tests/deflate_craft.py as BGZF
members — codes of up to 15 bits behind the kernel's 10 / 8-bit look-ups (its canonical walk), full alphabets, a lone distance
code and none, 7-bit code-length codes, repeats across HLIT, every length and distance symbol at both ends of its extra bits,
overlapping copies (the wave-wide j % dist), 120 tiny blocks per member; the write-out and the CRC slices at every text length
that changes their shape; every refusal the kernel's header comment promises; and one crafted file through hulk_sketch_files.
tests/test_deflate_crafted_cpu.py holds the same corpus against zlib and the host decoders."""
import numpy as np
import pytest

import deflate_craft as dc
from test_gpu_bgzf_device import _child_inflate, _dev_flags, _run, _same

pytestmark = pytest.mark.gpu
N_RANDOM = 120                                   # the slice of the random streams the CPU tests take 300 of


def test_valid_corpus_is_byte_exact(tmp_path):
    """every valid stream as one member: 25 members to a call, all of them in one call, and a FASTQ of crafted members built
    member by member (per-member token lists, records straddling them); the text byte for byte"""
    corpus = dc.valid_corpus(N_RANDOM)
    stats = dc.corpus_stats(corpus)
    assert stats["ll_max"] == 15 and stats["d_max"] == 15 and stats["lone"] >= 10 and stats["nodist"] >= 10, stats
    members = [dc.bgzf_member(c["text"], c["body"]) for c in corpus]
    groups = [list(range(a, min(a + 25, len(corpus)))) for a in range(0, len(corpus), 25)] + [list(range(len(corpus)))]
    cases = [b"".join(members[k] for k in g) for g in groups]
    fq_members, seqs, info = dc.fastq_bgzf_members(9, 600_000)
    assert info["members"] >= 10 and info["ll_max"] == 15
    cases.append(b"".join(fq_members))
    res = _child_inflate(tmp_path, cases)
    for i, (r, g) in enumerate(zip(res, groups)):
        assert r[0] == "ok", (i, r)
        at = 0
        for k in g:                                                        # (stream by stream, to name the one that differs)
            t = corpus[k]["text"]
            assert r[1][at:at + len(t)] == t, (i, corpus[k]["name"])
            at += len(t)
        assert at == len(r[1])
    assert res[-1][0] == "ok" and res[-1][1].split(b"\n")[1::4] == seqs


def _plain_member(text):
    """stored blocks where a BGZF member (at most 65,536 bytes, 26 of them header and trailer) has room for them; a text of more
    than 65,500 bytes cannot be stored in one: 60,000 stored bytes, then fixed-code matches copy the rest from 30,000 back"""
    st = dc.Stream()
    if len(text) <= 65500:
        return dc.bgzf_member(*st.stored(text, True).finish()[::-1])
    st.stored(text[:60000])
    rest, toks = len(text) - 60000, []
    while rest:
        n = rest if rest <= 258 else min(258, rest - 3)
        toks.append(("match", n, 30000)); rest -= n
    body, t = st.fixed(toks, True).finish()
    assert t == text
    return dc.bgzf_member(t, body)


def test_write_out_and_crc_slices(tmp_path):
    """one call: texts of 0..260, 1,021..1,030, 16,381..16,388, 65,277..65,283 and 65,533..65,536 bytes (the lengths at which
    the head / dwords / tail of the write-out and the 64 CRC slices change shape), every length up to 260 at every residue of
    out_off mod 4.  (Stored blocks, except 65,533..65,536: see _plain_member.)"""
    rng = np.random.default_rng(17)
    pool = rng.integers(0, 256, 60000, dtype=np.uint8).tobytes()
    pool = pool + pool[30000:30000 + 5536]                                 # (bytes 60,000.. repeat those 30,000 back)
    lengths, off, seen = [], 0, set()

    def put(n):
        nonlocal off
        lengths.append(n); seen.add((n, off % 4)); off += n
    for r in range(4):
        for n in range(261):
            if (n, r) in seen:
                continue
            if off % 4 != r:
                put((r - off) % 4)                                         # a filler of 1..3 bytes (a small length itself)
            put(n)
    for n in list(range(1021, 1031)) + list(range(16381, 16389)) + list(range(65277, 65284)) + list(range(65533, 65537)):
        put(n)
    assert all((n, r) in seen for n in range(261) for r in range(4))
    assert len({off % 4 for n, off in seen if n > 260}) == 4
    texts = [pool[(7 * i) % 100:(7 * i) % 100 + n] if n <= 65283 else pool[:n] for i, n in enumerate(lengths)]
    data = b"".join(_plain_member(t) for t in texts)
    res = _child_inflate(tmp_path, [data])
    assert res[0][0] == "ok", res[0]
    got, want = res[0][1], b"".join(texts)
    assert len(got) == len(want)
    if got != want:
        at = next(k for k in range(len(want)) if got[k] != want[k])
        ends = np.cumsum(lengths)
        k = int(np.searchsorted(ends, at, side="right"))
        raise AssertionError("byte %d differs: member %d of %d bytes at out_off %d" % (at, k, lengths[k], ends[k] - lengths[k]))


def test_malformed_members_are_refused_with_their_reason(tmp_path):
    """each malformed stream in the place of member 2 of five good ones: an error that names member 2 and carries status_text's
    reason for that defect — for the streams that are wrong in themselves the verdict is zlib's (it refuses every one of them);
    the five good members still inflate afterwards, in the same process"""
    good = [c for c in dc.valid_corpus(0) if 200 <= len(c["text"]) <= 20000][:5]
    assert len(good) == 5
    members = [dc.bgzf_member(c["text"], c["body"]) for c in good]
    table = dc.malformed_corpus()
    assert {m["status"] for m in table} == {dc.BAD_SYMBOL, dc.BAD_CODE, dc.STORED_LEN, dc.EXHAUSTED, dc.TOO_LONG, dc.TOO_SHORT, dc.TRAILING}
    cases = [b"".join(members[:2]) + dc.bgzf_member(m["text"], m["body"]) + b"".join(members[3:]) for m in table]
    cases.append(b"".join(members))
    res = _child_inflate(tmp_path, cases)
    start = len(members[0]) + len(members[1])
    for m, r in zip(table, res):
        assert (m["zlib"] == "reject") == (m["level"] == "deflate") and dc.zlib_verdict(m["body"])[0] == m["zlib"], m["name"]
        assert r[0] == "err", (m["name"], r[0])
        assert r[3] == 2 and r[2] == "bgzf: member 2 (byte %d): %s" % (start, m["status"]), (m["name"], r)
    assert res[-1] == ("ok", b"".join(c["text"] for c in good))


def test_sketch_path_on_crafted_members(tmp_path, capfd):
    """a BGZF FASTQ of crafted members (a few hundred KB, several 128 KiB blocks, records straddling members) through
    hulk_sketch_files: the same stats, sketch and counters with HULK_INGEST_DEVICE_INFLATE as without, every member inflated on
    the GPU, nothing handed over"""
    data, seqs, info = dc.fastq_bgzf(21, 500_000, lo=300, hi=40000)
    assert info["members"] >= 15 and info["ll_max"] == 15 and info["d_max"] >= 9
    p = str(tmp_path / "crafted.fq.gz")
    with open(p, "wb") as f:
        f.write(data)
    r0, r1 = _run([p], 0), _run([p], _dev_flags())
    assert r0[0] != "error" and r0[0][0] == len(seqs) and r0[0][1] == sum(len(s) for s in seqs)
    assert _same(r0, r1)
    err = capfd.readouterr().err
    assert "%d members inflated on the GPU" % (info["members"] + 1) in err and "handed over" not in err
