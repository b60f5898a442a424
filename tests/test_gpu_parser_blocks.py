"""The device FASTQ / FASTA parsers (hulk_fastq.hip) at the block sizes they ship with, and at the edges of their buffers.

hulk_sketch_files parses on the device in blocks of 16 MiB; the rest of the suite gives the FASTQ parser blocks of 128 KiB to
1 MiB, where each of its single-workgroup scans (k_fq_scan_u32, k_fq_scan_maps, k_fq_scan_cnt; k_fa_scan for --fasta) ends in its
first trip and the carry from trip to trip has never carried anything, and where k_fa_class / k_fa_flags / k_fa_emit never go round
their grid twice.  The inputs of tests/parser_inputs.py reach the third trip of every one of them (where `carry = total` first
differs from `carry += total`), with slot states other than 0 in front of the trip borders, and stand on the two limits that
hand a FASTQ block to the host parser: a tail of exactly the porch and one byte more, a range of exactly line_cap lines and one
more.  tests/test_parser_inputs_cpu.py holds the inputs to their conditions and to the host parser without a GPU.

Every case, three ways: hulk_sketch_files on the device parser, with HULK_INGEST_HOST_PARSER, and the generator's reads through
hulk_add_reads — the stats are the closed form, and mins, weight bits, count-min counters and counters are equal.  A dropped,
doubled or shifted read changes the count-min counters; the interval makes a reordering across a border change the sketch.  The
device run is traced: where the device's result must stand, a run that the host parser took over (and got right) is a failure."""
import numpy as np
import pytest

import parser_inputs as pi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def release_the_parser_buffers():
    """behind the module's last test: the 24 MiB buffer set (and the 8 MiB one) do not stay pinned for the rest of the suite"""
    yield
    from hulk_amd import _lib
    assert _lib.load().hulk_release_caches() == 0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def results(g, stats=None):
    m, w = g.sketch()
    return dict(stats=stats, mins=m, weights=w, cms=g.cms(), counters=g.counters())


def run_files(c, flags):
    import hulk_amd
    g = hulk_amd.GpuSketcher(pi.K, pi.W, pi.S, interval=c.interval)
    try:
        opts = {"flags": flags}
        if c.block_bytes:
            opts["block_bytes"] = c.block_bytes
        st = g.sketch_files([c.path], fasta=c.fasta, opts=opts)
        g.finish()
        return results(g, (st["n_seqs"], st["total_len"], st["n_lines"]))
    finally:
        g.close()


def run_reads(c):
    import hulk_amd
    g = hulk_amd.GpuSketcher(pi.K, pi.W, pi.S, interval=c.interval)
    try:
        g.add_reads(c.bases, c.offsets)
        g.finish()
        return results(g)
    finally:
        g.close()


def assert_same(a, b, what):
    assert np.array_equal(a["mins"], b["mins"]), f"{what}: mins"
    assert np.array_equal(bits(a["weights"]), bits(b["weights"])), f"{what}: weights"
    assert np.array_equal(a["cms"], b["cms"]), f"{what}: count-min counters, {int((a['cms'] != b['cms']).sum())} differ"
    assert a["counters"] == b["counters"], f"{what}: counters {a['counters']} {b['counters']}"


@pytest.mark.parametrize("name", pi.CASES)
def test_device_parser_host_parser_and_add_reads_agree(name, tmp_path, capfd):
    from hulk_amd import _lib
    c = pi.build(name, tmp_path)
    m = c.check()
    capfd.readouterr()
    dev = run_files(c, _lib.HULK_INGEST_TRACE)
    trace = capfd.readouterr().err                                      # (the library writes the trace to the process's stderr)
    print(f"{c.name}: block {c.block}, interval {c.interval}, {len(m.data)} bytes, stats {c.stats}\n{m.report()}")
    print(trace.strip())
    assert "ingest trace (device FAST" + ("A" if c.fasta else "Q") + " parser" in trace, "the device parser did not run"
    host = run_files(c, _lib.HULK_INGEST_HOST_PARSER)
    want = run_reads(c)
    print("stats: device", dev["stats"], "host parser", host["stats"], "closed form", c.stats, "counters", dev["counters"], want["counters"])
    if not c.fasta:                                                     # (the FASTA parser has no hand-over)
        if c.takeover:
            assert "host parser took over" in trace, "the device's result stood beyond the limit"
        else:
            assert "host parser took over" not in trace, "the device handed a block it has to parse itself to the host parser"
    assert host["stats"] == c.stats, "host parser: stats"
    assert_same(host, want, "host parser against hulk_add_reads")
    assert dev["stats"] == c.stats, "device parser: stats"
    assert_same(dev, want, "device parser against hulk_add_reads")
    assert_same(dev, host, "device parser against host parser")
    assert want["counters"]["n_reads"] == c.stats[0] and want["counters"]["total_len"] == c.stats[1]
