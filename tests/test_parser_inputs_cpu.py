"""The inputs of tests/parser_inputs.py, checked without a GPU.

tests/test_gpu_parser_blocks.py runs these files through the device parsers; what makes them bite — a scan that carries into its
third trip, a slot state other than 0 at a trip border, a tail of exactly the porch, a range of exactly line_cap lines — is a
property of the input, of the block size and of constants of hulk_fastq.hip / hulk_ingest_device.hip.  Pinned here: the constants
against the source text (a changed trip width fails a test, it does not quietly turn the inputs into single-trip ones), every
case's condition, and the generators' reads and stats against two implementations they did not come from: the host parser
(hulk_parse_files) at full size and the literal restatement oracle/linepump.py (cases 1 and 3 at 1/50 of their size: it is a
Python loop over lines)."""
import os

import numpy as np
import pytest

import parser_inputs as pi

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hulk_amd", "csrc")


def test_the_constants_follow_the_sources():
    fq = open(os.path.join(CSRC, "hulk_fastq.hip")).read()
    dev = open(os.path.join(CSRC, "hulk_ingest_device.hip")).read()
    hdr = open(os.path.join(CSRC, "hulk_fastq.h")).read()
    assert "constexpr int FQ_T = 256;" in fq and pi.FQ_T == 256
    assert "constexpr uint32_t FQ_CHUNK = FQ_T * 16;" in fq and pi.FQ_CHUNK == pi.FQ_T * 16 == 4096
    assert "const uint32_t addr = a0 + blockIdx.x * FQ_CHUNK + threadIdx.x * 16u;" in fq and pi.THREAD_BYTES == 16
    assert "const uint32_t lo = st->start, hi = st->end, a0 = lo & ~15u;" in fq
    assert "constexpr int FA_T = FQ_T;" in fq and "constexpr uint32_t FA_CHUNK = FQ_CHUNK;" in fq and pi.FA_T == pi.FQ_T
    # the trips: 8 entries a thread in the three FASTQ scans, 16 in k_fa_scan
    assert fq.count("base += 8u * FQ_T)") == 3 and fq.count("const uint32_t at = base + threadIdx.x * 8 + i;") == 6 and pi.FQ_TRIP == 8 * 256
    assert fq.count("base += 16u * FA_T)") == 1 and fq.count("const uint32_t at = base + threadIdx.x * 16 + i;") == 2 and pi.FA_TRIP == 16 * 256
    for kernel, trip in (("k_fq_scan_u32", "8u * FQ_T"), ("k_fq_scan_maps", "8u * FQ_T"), ("k_fq_scan_cnt", "8u * FQ_T"), ("k_fa_scan", "16u * FA_T")):
        body = fq[fq.index("void " + kernel + "("):]
        assert "base += " + trip in body[:body.index("\n}\n")], kernel
    # the grids of a block
    assert fq.count("const uint32_t span = B.porch + len + 16u;") == 2 and pi.span(5) == pi.PORCH + 21
    assert "const uint32_t nchunks = (span + FQ_CHUNK - 1) / FQ_CHUNK;" in fq and "const uint32_t nchunks = (span + FA_CHUNK - 1) / FA_CHUNK;" in fq
    assert "const uint32_t nlwg = (B.line_cap + FQ_T - 1) / FQ_T;" in fq and "const uint32_t nlwg = (B.line_cap + FA_T - 1) / FA_T;" in fq
    assert "const uint32_t glw = std::min<uint32_t>(nlwg, (span / 16u + FA_T - 1) / FA_T + 1u);" in fq
    assert "for (uint32_t i = blockIdx.x * FA_T + threadIdx.x; i < NL; i += gridDim.x * FA_T) {" in fq
    assert fq.count("for (uint32_t blk = blockIdx.x; blk * FA_T < ev; blk += gridDim.x) {") == 2
    # the limits
    assert "const bool fits = tl <= porch;" in fq
    assert "if (carry > cap) { st->need_host |= FQ_NEED_LINES; carry = cap; }" in fq and "if (at < cap) line_end[at] = addr + b;" in fq
    assert "constexpr uint32_t FQ_MAX_TOKEN = 64 * 1024;" in hdr and pi.MAX_TOKEN == 65536
    # the buffers and the block size
    assert "d->porch = 1u << 20;" in dev and pi.PORCH == 1 << 20
    assert "B.line_cap = (uint32_t)((d->porch + block) / 8 + 1024);" in dev and "B.read_cap = B.line_cap / 2;" in dev
    assert "B.bytes_cap = d->porch + block;" in dev
    assert "const uint32_t line_cap = (uint32_t)((MAX_TOKEN + D->block) / 2 + 2);" in dev
    assert "if (!cfg.block_set) cfg.block = (size_t)16u << 20;" in dev and pi.DEFAULT_BLOCK == 16 << 20
    assert "D = fq_dev_for(ctx, std::min<size_t>(cfg.block, (size_t)32u << 20), err);" in dev and pi.MAX_BLOCK == 32 << 20
    assert "while (have < dev_->block) {" in dev                      # the reader fills a block to its last byte
    # what the issue's figures come to
    assert pi.fq_line_cap(131072) == 148_480 and pi.fq_line_cap(16 << 20) == 2_229_248 and pi.fa_line_cap(16 << 20) == 8_421_378
    assert pi.n_chunks(16 << 20) == 4353 and pi.fq_line_wgs(16 << 20) == 8708 and pi.n_chunks(131072) == 289 and pi.fq_line_wgs(131072) == 580
    assert pi.FQ_TRIP_LINES == 524_288 and pi.FA_TRIP_LINES == 1_048_576
    assert pi.fa_glw(16 << 20, 16 << 20) == 4354 and pi.fa_glw(131072, 131072) == 290


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("parser_inputs")


_CASES = {}


def case(name, workdir):
    if name not in _CASES:
        _CASES[name] = pi.build(name, workdir)
    return _CASES[name]


@pytest.mark.parametrize("name", pi.CASES)
def test_the_case_is_a_test_and_the_host_parser_reads_what_it_claims(name, workdir):
    """the case's condition holds on the model; hulk_parse_files returns exactly the generator's reads and stats"""
    from hulk_amd import ingest
    c = case(name, workdir)
    m = c.check()
    print(f"{c.name}: block {c.block}, {os.path.getsize(c.path)} bytes\n{m.report()}")
    bases, offsets, st = ingest.parse_files([c.path], fasta=c.fasta, opts={"block_bytes": c.block_bytes} if c.block_bytes else None)
    assert (st["n_seqs"], st["total_len"], st["n_lines"]) == c.stats
    assert np.array_equal(offsets, c.offsets) and np.array_equal(bases, c.bases)


def test_the_trips_the_cases_are_meant_to_take(workdir):
    """three trips or more of every scan named in cases 1 to 3, in the model's count"""
    c = case("fastq_line_scans", workdir)
    m = c.model()
    good = pi.check_line_scans(c, m)
    assert all(m.line_trips(b) >= 3 for b in good) and max(m.byte_trips(b) for b in range(m.n_blocks)) >= 3
    m = case("fastq_byte_scan", workdir).model()
    assert m.byte_trips(0) == 3
    for name in ("fasta_trips", "fasta_trips_crlf"):
        c = case(name, workdir)
        m = c.model()
        good = pi.check_fasta_trips(c, m)
        assert all(m.fa_scan_trips(b) >= 3 and m.fa_grid_rounds(b) >= 4 for b in good)


def test_a_condition_that_does_not_hold_fails(tmp_path):
    """the checks refuse inputs that do not do what they claim: clean four-line records carry slot state 0 to every trip border, and
    at 1/50 of its size no case reaches a second trip"""
    n = (2 * pi.DEFAULT_BLOCK + 6_500_000) // 37
    bases, offsets = pi._reads(0, n, 15)
    p = str(tmp_path / "clean.fq")
    pi._fastq_rows(bases, n, 15).tofile(p)
    clean = pi.Case("clean", p, False, 0, 4000, bases, offsets, (n, n * 15, 4 * n), pi.check_line_scans)
    with pytest.raises(AssertionError, match="the inputs are no test: no block whose slot states"):
        clean.check()
    small = pi.fasta_short_lines(str(tmp_path / "small.fa"), 12_000)
    with pytest.raises(AssertionError, match="the inputs are no test: no block with more than"):
        small.check()


@pytest.mark.parametrize("name", pi.CASES)
def test_the_line_pump_reads_the_same(name, tmp_path, workdir):
    """oracle/linepump.py, the literal restatement of the reference's line machine, on the generator's file"""
    from oracle import linepump
    c = pi.build(name, tmp_path, scale=50) if name in pi.SCALED else case(name, workdir)
    if name in pi.SCALED:
        c.check()                                            # (the closed forms against the file; the trips are the full size's)
    want = linepump.sequences([c.path], fasta=c.fasta)
    assert len(want) == c.stats[0]
    got = c.bases.tobytes()
    off = c.offsets.astype(np.int64)
    assert b"".join(want) == got and [len(s) for s in want] == np.diff(off).tolist()
