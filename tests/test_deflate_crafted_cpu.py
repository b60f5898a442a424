"""The host DEFLATE decoders on streams zlib's encoder never writes (tests/deflate_craft.py): hulk::inflate::Decoder
(fast_inflate.h) and the symbol decoder of par_inflate.h through tests/cpp/inflate_fuzz.cpp --corpus, plain and under
-fsanitize=address,undefined (a program of its own: nothing is preloaded), and the file readers on FASTQ files made of many
small dynamic blocks of deep codes.  The helper has checked every valid stream against zlib.decompressobj(-15) before it hands
it out; the verdicts recorded beside the malformed ones are checked here."""
import hashlib
import json
import os
import struct
import subprocess
import sys

import pytest

import deflate_craft as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 300


@pytest.fixture(scope="module")
def corpus():
    return dc.valid_corpus(N_RANDOM), dc.malformed_corpus()


def test_helper_shapes_and_self_check():
    """the code shapes are complete sets within their limits, the repeat coding gives back the lengths it was given, and a
    stream that does not inflate to its text cannot leave the helper"""
    import random
    rng = random.Random(5)
    assert dc.deepest_lengths(16) == list(range(1, 16)) + [15] and dc.deepest_lengths(2) == [1, 1]
    for n in list(range(2, 40)) + [100, 286]:
        for lens in (dc.deepest_lengths(n), dc.random_lengths(n, rng), dc.random_lengths(n, rng, chain=1.0), dc.balanced_lengths(n)):
            assert len(lens) == n and max(lens) <= 15 and dc.kraft(lens) == 1 << 15
    for n in range(2, 20):
        for lens in (dc.deepest_lengths(n, 7), dc.random_lengths(n, rng, 7)):
            assert len(lens) == n and max(lens) <= 7 and dc.kraft(lens, 7) == 1 << 7
    assert max(dc.deepest_lengths(286)) == 15 and max(dc.deepest_lengths(30)) == 15 and max(dc.deepest_lengths(19, 7)) == 7
    for _ in range(200):
        seq = [rng.choice((0, 0, 0, 3, 7, 7, 7, 15)) for _ in range(rng.randint(1, 316))]
        assert dc.ops_lengths(dc.rle_ops(seq)) == seq and dc.ops_lengths(dc.rle_ops(seq, rng)) == seq
    assert dc.len_symbol(258) == (285, 0, 0) and dc.len_symbol(257) == (284, 5, 30) and dc.dist_symbol(32768) == (29, 13, 8191)
    assert dc.expand([("match", 7, 2)], b"ab") == b"ababababa"
    st = dc.Stream("lying").fixed(dc.lits(b"ACGT"), True)
    st.text += b"!"                                                         # (the text no longer is what the tokens expand to)
    with pytest.raises(AssertionError, match="zlib disagrees"):
        st.finish()
    with pytest.raises(AssertionError, match="no final block"):
        dc.Stream().fixed([]).finish()


def test_corpus_reaches_the_paths_it_is_for(corpus):
    """codes of 15 bits on both alphabets, beyond the primary look-ups of every decoder (11 / 8 bits on the host, 10 / 8 in the
    kernel); lone and absent distance codes; repeats across HLIT; 7-bit code-length codes; every planned case in every encoding;
    and the recorded zlib verdict of every malformed stream is zlib's"""
    valid, malformed = corpus
    s = dc.corpus_stats(valid)
    print("corpus:", json.dumps(s))
    assert s["ll_max"] == 15 and s["d_max"] == 15
    assert s["lone"] >= 10 and s["nodist"] >= 10 and s["cross"] >= 10 and s["clc7"] >= 10
    assert s["ll_over_11"] >= 50 and s["d_over_8"] >= 50
    assert all(len(c["text"]) <= 65536 and len(c["body"]) + 26 <= 65536 for c in valid)
    names = {c["name"] for c in valid}
    for name, _, codes in dc.planned_token_lists():
        for how in dc.ENCODINGS:
            assert (name + "/" + how in names) == (how != "fixed" or not codes), (name, how)
    mix = [c for c in valid if c["name"].startswith("block mix")]
    assert len(mix) == 2 and all(c["info"]["blocks"] == 120 for c in mix)
    # length symbols: both ends of every symbol's extra bits; distance symbols likewise, up to 32,768
    toks = dict((n, b) for n, b, _ in dc.planned_token_lists())
    lens = {t[1] for t in toks["length symbols"][0] if t[0] == "match"}
    assert lens >= {dc.LEN_BASE[i] + x for i in range(29) for x in (0, (1 << dc.LEN_EXTRA[i]) - 1)} and 258 in lens
    dists = {t[2] for t in toks["distance symbols"][0] if t[0] == "match"}
    assert dists >= {dc.DIST_BASE[i] + x for i in range(30) for x in (0, (1 << dc.DIST_EXTRA[i]) - 1)} and 32768 in dists
    over = {(t[1], t[2]) for name in toks if name.startswith("overlap") for t in toks[name][0] if t[0] == "match"}
    for d in list(range(1, 71)) + [127, 128, 129, 255, 256, 257]:
        for n in (3, 4, d, d + 1, 63, 64, 65, 127, 128, 129, 257, 258):
            assert not 3 <= n <= 258 or (n, d) in over, (n, d)
    assert len(malformed) == 23
    for m in malformed:
        verdict, text = dc.zlib_verdict(m["body"])
        assert verdict == m["zlib"], m["name"]
        assert (m["level"] == "member") == (verdict == "accept"), m["name"]


def _corpus_file(path, valid, malformed):
    def rec(kind, name, body, text):
        name = name.encode()
        return bytes([kind]) + struct.pack("<I", len(name)) + name + struct.pack("<I", len(body)) + body + struct.pack("<I", len(text)) + text
    with open(path, "wb") as f:
        for c in valid:
            f.write(rec(0, c["name"], c["body"], c["text"]))
        for m in malformed:                                                # zlib's verdict: refused -> ERROR, inflated -> DONE with that text
            verdict, text = dc.zlib_verdict(m["body"])
            f.write(rec(1 if verdict == "reject" else 2, m["name"], m["body"], text or b""))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_streams_against_both_host_decoders(tmp_path, corpus, sanitize):
    """every valid stream through Decoder at input pieces 1 / 7 / 300 / 2^20 against output pieces 1 / 600 / 2^22 and through the
    fuzzer's spec_check; every malformed one gets zlib's verdict; once more as a sanitized build of the same program"""
    valid, malformed = corpus
    path = str(tmp_path / "corpus.bin")
    _corpus_file(path, valid, malformed)
    exe = str(tmp_path / "inflate_fuzz")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"] if sanitize else ["-O2"]
    subprocess.run(["g++"] + flags + ["-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "cpp", "inflate_fuzz.cpp"), "-lz"],
                   check=True, timeout=300)
    r = subprocess.run([exe, "--corpus", path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    n_member = sum(1 for m in malformed if m["level"] == "member")
    assert "corpus: %d streams (%d valid, %d refused, %d accepted with a flaw around them), 0 bad" % (
        len(valid) + len(malformed), len(valid), len(malformed) - n_member, n_member) in r.stdout


def _children(paths, **env):
    """tools/fuzz_gzpar.py --child in a fresh process: {path: [n_seqs, md5(bases), md5(offsets)] or ["error", message]}, stderr"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_gzpar.py"), "--child"] + paths, capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, HULK_INGEST_TRACE="1", **env))
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("[")]
    assert len(rows) == len(paths), r.stderr[-2000:]
    return {row[0]: row[1:] for row in rows}, r.stderr


def test_file_readers_on_crafted_fastq(tmp_path):
    """a one-member .gz and a BGZF file of random member sizes, each a FASTQ of a few MB in small dynamic blocks of deep codes:
    the parallel readers (small chunks, 3 threads), the one-thread reader and zlib's inflate give the reads of the text; the
    parallel reader counted chunks on the one-member file; a malformed member in the middle of the BGZF file gives the same
    message with the member threads as without"""
    gz, seqs_gz, info = dc.fastq_gzip(3, 2_500_000)
    bg, seqs_bg, info_bg = dc.fastq_bgzf(4, 2_500_000)
    assert info["ll_max"] == 15 and info["d_max"] == 15 and info["blocks"] > 2000 and info_bg["members"] > 40
    bad = next(m for m in dc.malformed_corpus() if m["name"] == "fixed-code symbol 286")
    broken, _, _ = dc.fastq_bgzf(4, 2_500_000, bad_member=(info_bg["members"] // 2, bad["body"], bad["text"]))
    assert broken != bg and broken[:100000] == bg[:100000]
    p_gz, p_bg, p_bad = (str(tmp_path / n) for n in ("one.fq.gz", "members.fq.gz", "broken.fq.gz"))
    for p, data in ((p_gz, gz), (p_bg, bg), (p_bad, broken)):
        with open(p, "wb") as f:
            f.write(data)
    want = {p_gz: [len(seqs_gz), hashlib.md5(b"".join(seqs_gz)).hexdigest()], p_bg: [len(seqs_bg), hashlib.md5(b"".join(seqs_bg)).hexdigest()]}
    legs = [_children([p_gz, p_bg, p_bad], **env) for env in ({"HULK_GZ_PAR_CHUNK": "65536", "HULK_GZ_THREADS": "3"}, {"HULK_GZ_PAR": "0"},
                                                              {"HULK_GZ_ZLIB": "1"})]
    for res, _ in legs:
        for p in (p_gz, p_bg):
            assert res[p][:2] == want[p], (p, res[p])
        assert res[p_gz] == legs[0][0][p_gz] and res[p_bg] == legs[0][0][p_bg]
    trace = [l for l in legs[0][1].splitlines() if "parallel gzip reader," in l]
    assert len(trace) == 1 and "parallel gzip reader," not in legs[1][1]
    assert int(trace[0].split(" chunks counted")[0].split()[-1]) >= 10, trace
    assert "BGZF reader, %d members inflated" % (info_bg["members"] + 1) in legs[0][1]
    one, _ = _children([p_bad], HULK_GZ_THREADS="1")
    assert legs[0][0][p_bad][0] == "error" and legs[0][0][p_bad] == legs[1][0][p_bad] == one[p_bad], (legs[0][0][p_bad], one[p_bad])
