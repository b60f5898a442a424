"""The KMV and KHF MinHash sketches fed on the GPU (HULK_FLAG_KMV / HULK_FLAG_KHF, hulk_get_minhash, hulk_minhash_merge).

Reference for every comparison: the numpy restatement of src/minhash/kmv.go:39-71 / khf.go:34-45 in tests/test_minhash_cpu.py,
fed with what the boss's collector feeds the k-mer spectrum (src/pipeline/boss.go:90-95): the distinct minimizer values of every
read, oracle.pyorc.minimizers(read, k, w).  Both sketches are order-independent, so every comparison is array_equal."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, pack_reads
from minhash_inputs import U64_MAX, fed_values, khf_merge_reference, khf_reference, kmv_reference, n_reads
from oracle import pyorc

pytestmark = pytest.mark.gpu

W = 9
LIBDIR = os.path.join(ROOT, "hulk_amd", "csrc")


def flags_both():
    from hulk_amd import _lib
    return _lib.HULK_FLAG_KMV | _lib.HULK_FLAG_KHF


def sketcher(k, S, w=W, **kw):
    import hulk_amd
    kw.setdefault("flags", flags_both())
    return hulk_amd.GpuSketcher(k, w, S, **kw)


def assert_minhash(g, vals, S, what=""):
    from hulk_amd import _lib
    kmv, fed = g.minhash(_lib.HULK_MINHASH_KMV)
    khf, fed2 = g.minhash(_lib.HULK_MINHASH_KHF)
    want_kmv, want_khf = kmv_reference(vals, S), khf_reference(vals, S)
    assert fed == fed2 == len(vals) == g.counters()["n_minimizers"], what
    assert len(kmv) == min(S, len(vals)), what
    assert np.array_equal(kmv, want_kmv), f"{what}: KMV differs in {int((kmv != want_kmv).sum())} of {len(kmv)} entries"
    assert len(khf) == S and np.array_equal(khf, want_khf), f"{what}: KHF differs in {int((khf != want_khf).sum())} of {S} slots"
    return kmv, khf


@pytest.mark.parametrize("S", [1, 50, 512, 1024])
@pytest.mark.parametrize("k", [21, 27, 31])
def test_fixture_reads(fq_reads, k, S):
    """k = 21: no product can wrap, the KHF feed is a min-reduction; k = 27 / 31: almost every slot differs from (i+1) * min(x)."""
    bases, offsets = pack_reads(fq_reads)
    vals = fed_values(bases, offsets, k)
    g = sketcher(k, S)
    g.add_reads(bases, offsets)
    _, khf = assert_minhash(g, vals, S, f"k={k} S={S}")
    with np.errstate(over="ignore"):
        naive = vals.min() * np.arange(1, S + 1, dtype=np.uint64)
    if k == 21:
        assert np.array_equal(khf, naive)
    elif S >= 512:
        assert int((khf != naive).sum()) > S // 2           # the wrap really decides slots here
    if k == 21 and S in (50, 512):
        assert len(np.unique(kmv_reference(vals, S))) < S   # the fixture exercises the multiset rule
    g.finish()
    assert_minhash(g, vals, S, "after finish")              # getters work on a finished context
    g.close()


def test_fewer_values_than_slots_and_an_empty_context(fq_reads):
    from hulk_amd import _lib
    bases, offsets = pack_reads(fq_reads[:3])
    vals = fed_values(bases, offsets, 27)
    assert 0 < len(vals) < 512
    g = sketcher(27, 512)
    kmv, fed = g.minhash(_lib.HULK_MINHASH_KMV)
    khf, _ = g.minhash(_lib.HULK_MINHASH_KHF)
    assert len(kmv) == 0 and fed == 0 and khf.tolist() == [U64_MAX] * 512
    g.add_reads(bases, offsets)
    kmv, _ = assert_minhash(g, vals, 512)
    assert len(kmv) == len(vals) < 512
    g.close()


@pytest.mark.parametrize("k", [21, 31])
def test_every_binning_path(k):
    """short reads with N (deferred to the generic kernel), 600- and 1000-base reads (the generic kernel alone), 5-kb reads and one
    300-kb contig whose workgroups loop over tiles (the long path), a batch mixing all of them, and synthetic reads"""
    from hulk_amd import synth
    from test_gpu_long_tiles import grouped_input
    S = 512
    cases = {
        "short with N": pack_reads(n_reads(1, 3000, 100, 150, n_frac=0.3)),
        "600 and 1000 bases": pack_reads(n_reads(2, 300, 600, 600) + n_reads(3, 200, 1000, 1000, n_frac=0.2)),
        "long": grouped_input(4, k, W, 2000, (5000, 5200), [300000], [0.5], tail=0)[:2],
        "mixed": pack_reads(n_reads(5, 500, 100, 150, n_frac=0.2) + n_reads(6, 50, 600, 1000) + n_reads(7, 20, 5000, 9000) +
                            n_reads(8, 1, 300000, 300000) + n_reads(9, 500, 100, 300)),
        "synthetic": synth.reads_numpy(0, 20000, 150),
    }
    g_all, all_vals = sketcher(k, S), []
    for name, (bases, offsets) in cases.items():
        vals = fed_values(bases, offsets, k)
        g = sketcher(k, S)
        g.add_reads(bases, offsets)
        assert_minhash(g, vals, S, f"{name} k={k}")
        g.close()
        g_all.add_reads(bases, offsets)
        all_vals.append(vals)
    assert_minhash(g_all, np.concatenate(all_vals), S, f"all cases in one context k={k}")
    g_all.close()


@pytest.mark.parametrize("k", [21, 27])
def test_order_and_batching_independence(fq_reads, k):
    import torch
    S = 128           # (two 64-entry chunks of the KMV array; a context's CWS tables grow with S, and this test creates many)
    reads = fq_reads + n_reads(12, 400, 100, 150, n_frac=0.2) + n_reads(13, 30, 600, 900)
    bases, offsets = pack_reads(reads)
    vals = fed_values(bases, offsets, k)
    want = None
    for per_call in (len(reads), 1000, 7, 1):
        for lanes, interval, batch in ((1, 0, 16), (2, 0, 16), (2, 100, 1), (1, 100, 16), (2, 100, 16)):
            if per_call == 1 and (lanes, interval, batch) != (2, 100, 16):
                continue
            for device in (False, True):
                if device and per_call < 1000:
                    continue
                g = sketcher(k, S, interval=interval, work_lanes=lanes, batch=batch)
                for a in range(0, len(reads), per_call):
                    b = min(len(reads), a + per_call)
                    pb, po = pack_reads(reads[a:b])
                    if device:
                        tb = torch.from_numpy(np.concatenate([pb, np.zeros(16, np.uint8)])).cuda()
                        to = torch.from_numpy(po.astype(np.int64)).cuda()
                        torch.cuda.synchronize()
                        g.add_reads_device(tb.data_ptr(), to.data_ptr(), b - a, max(len(r) for r in reads[a:b]), tb.numel())
                        g.synchronize()
                    else:
                        g.add_reads(pb, po)
                got = assert_minhash(g, vals, S, f"per_call={per_call} lanes={lanes} interval={interval} batch={batch} device={device}")
                if want is None:
                    want = got
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
                g.close()


def steady_reads(n, first=0):
    import torch
    from hulk_amd import synth
    tb, to = synth.reads_torch(first, n, 150)
    torch.cuda.synchronize()
    return tb, to


def test_steady_state_two_million_reads():
    """2^21 synthetic 150-bp reads, k = 21, S = 512, interval 32768 x batch 16: four batches alternate over the two work lanes, and
    from the second one on almost every value fails the KMV bound (the threshold path after warm-up)."""
    from hulk_amd import synth
    n, k, S, interval = 1 << 21, 21, 512, 32768
    g = sketcher(k, S, interval=interval, work_lanes=2, batch=16)
    assert n // (interval * g.batch_size) >= 4
    tb, to = steady_reads(n)
    g.add_reads_device(tb.data_ptr(), to.data_ptr(), n, 150, tb.numel())
    g.synchronize()
    kmv, khf = [], np.full(S, U64_MAX, dtype=np.uint64)
    total = 0
    for first in range(0, n, 1 << 17):                      # the reference, a slice of the stream at a time
        v = fed_values(*synth.reads_numpy(first, 1 << 17, 150), k)
        total += len(v)
        kmv = kmv_reference(np.concatenate([kmv, v]) if len(kmv) else v, S)
        khf = khf_merge_reference(khf, khf_reference(v, S))
    from hulk_amd import _lib
    got_kmv, fed = g.minhash(_lib.HULK_MINHASH_KMV)
    got_khf, _ = g.minhash(_lib.HULK_MINHASH_KHF)
    assert fed == total == g.counters()["n_minimizers"]
    assert np.array_equal(got_kmv, kmv) and np.array_equal(got_khf, khf)
    g.close()


def test_brute_force_khf_fifty_thousand_reads():
    """k = 31, S = 1024: every value updates every slot (about 10^9 slot updates), many workgroups"""
    from hulk_amd import synth
    n, k, S = 50000, 31, 1024
    g = sketcher(k, S, interval=10000, decay_ratio=0.02)
    tb, to = steady_reads(n, first=777)
    g.add_reads_device(tb.data_ptr(), to.data_ptr(), n, 150, tb.numel())
    g.synchronize()
    assert_minhash(g, fed_values(*synth.reads_numpy(777, n, 150), k), S)
    g.close()


def test_the_main_path_is_undisturbed(fq_reads):
    from hulk_amd import _lib
    from hulk_amd._lib import HulkError
    reads = fq_reads + n_reads(21, 200, 100, 150, n_frac=0.3) + n_reads(22, 20, 600, 3000)
    bases, offsets = pack_reads(reads)
    for k, decay, interval in ((21, 1.0, 250), (31, 0.05, 0)):          # (k = 31: an interval of 250 reads fills < 1 % of the bins)
        out = []
        for flags in (0, flags_both()):
            g = sketcher(k, 64, interval=interval, decay_ratio=decay, flags=flags)
            g.add_reads(bases, offsets)
            hist, ctr = g.histogram(), g.counters()
            g.finish()
            out.append((g.sketch(), hist, ctr, g.cms()))
            if not flags:
                for algo in (_lib.HULK_MINHASH_KMV, _lib.HULK_MINHASH_KHF):
                    with pytest.raises(HulkError) as e:
                        g.minhash(algo)
                    assert e.value.code == -34 and "created without HULK_FLAG_K" in e.value.message
                    with pytest.raises(HulkError) as e:
                        g.minhash_merge(algo, np.zeros(64, dtype=np.uint64))
                    assert e.value.code == -34
            g.close()
        (s0, h0, c0, m0), (s1, h1, c1, m1) = out
        assert np.array_equal(s0[0], s1[0]) and np.array_equal(s0[1], s1[1])
        assert np.array_equal(h0, h1) and c0 == c1 and np.array_equal(m0, m1)
    # one flag only: the other getter says so
    g = sketcher(21, 16, flags=_lib.HULK_FLAG_KMV)
    with pytest.raises(HulkError) as e:
        g.minhash(_lib.HULK_MINHASH_KHF)
    assert e.value.code == -34
    with pytest.raises(HulkError) as e:
        g.minhash(7)
    assert e.value.code == -30
    g.close()


@pytest.mark.parametrize("k", [21, 31])
def test_merge_of_two_halves_is_the_whole(fq_reads, k):
    from hulk_amd import _lib
    from hulk_amd._lib import HulkError
    S = 256
    reads = fq_reads + n_reads(31, 100, 600, 800)
    bases, offsets = pack_reads(reads)
    vals = fed_values(bases, offsets, k)
    half = len(reads) // 2
    a, b = sketcher(k, S), sketcher(k, S)
    a.add_reads(*pack_reads(reads[:half]))
    b.add_reads(*pack_reads(reads[half:]))
    for algo in (_lib.HULK_MINHASH_KMV, _lib.HULK_MINHASH_KHF):
        a.minhash_merge(algo, b.minhash(algo)[0])
    kmv, fed = a.minhash(_lib.HULK_MINHASH_KMV)
    khf, _ = a.minhash(_lib.HULK_MINHASH_KHF)
    assert fed == len(fed_values(*pack_reads(reads[:half]), k))          # AddHash calls of THIS context
    assert np.array_equal(kmv, kmv_reference(vals, S)) and np.array_equal(khf, khf_reference(vals, S))
    # a short KMV signature into an empty context: held = what was merged
    c = sketcher(k, S)
    c.minhash_merge(_lib.HULK_MINHASH_KMV, np.array([9, 3, 3], dtype=np.uint64))
    assert c.minhash(_lib.HULK_MINHASH_KMV)[0].tolist() == [3, 3, 9]
    with pytest.raises(HulkError) as e:
        c.minhash_merge(_lib.HULK_MINHASH_KHF, np.zeros(S - 1, dtype=np.uint64))
    assert e.value.code == -30
    for g in (a, b, c):
        g.close()


def test_cli_feed_minhash_end_to_end(tmp_path, fq_reads):
    import hashlib
    from hulk_amd.__main__ import main
    from hulk_amd.sketchio import load_hulk_data
    k, S = 27, 64
    halves = (fq_reads[:500], fq_reads[500:])
    d = tmp_path / "sk"
    d.mkdir()
    ref = {"kmv": [], "khf": []}
    for i, reads in enumerate(halves):
        fq = tmp_path / f"r{i}.fq"
        fq.write_bytes(b"".join(b"@r\n" + r + b"\n+\n" + b"I" * len(r) + b"\n" for r in reads))
        assert main(["sketch", "-f", str(fq), "-k", str(k), "-s", str(S), "--kmv", "--khf", "--feedMinHash", "-o", str(d / f"s{i}")]) == 0
        vals = fed_values(*pack_reads(reads), k)
        ref["kmv"].append(kmv_reference(vals, S)); ref["khf"].append(khf_reference(vals, S))
        doc = json.load(open(d / f"s{i}.json"))
        assert [s["Algorithm"] for s in doc["signatures"]] == ["histosketch", "kmv", "khf"]           # sketch.go:226-234
        for sig, algo in zip(doc["signatures"][1:], ("kmv", "khf")):
            assert list(sig["Sketch"]) == ["ksize", "md5sum", "mins", "num"]
            assert sig["Sketch"]["ksize"] == k and sig["Sketch"]["num"] == S
            assert sig["Sketch"]["mins"] == ref[algo][i].tolist()
        load_hulk_data(str(d / f"s{i}.json"))
    for algo in ("kmv", "khf"):
        out = str(tmp_path / f"m_{algo}")
        assert main(["smash", "-d", str(d), "-k", str(k), "-a", algo, "-o", out]) == 0
        rows = open(out + ".hulk-matrix.csv").read().strip().splitlines()
        got = [r.split(",") for r in rows[1:]]
        dist = pyorc.smash_matrix(np.stack(ref[algo]), np.zeros((2, S)))
        want = [["%.2f" % (100 - 100 * dist[s, q]) for q in range(2)] for s in range(2)]
        assert got == want and got[0][0] == got[1][1] == "100.00"
    # without --feedMinHash: what tests/test_gpu_parity.py::test_cli_khf_kmv_stream_flags pins
    fq = os.path.join(GOLDEN, "test-reads-small.fq.gz")
    out = str(tmp_path / "a")
    assert main(["sketch", "-f", fq, "-s", "16", "--khf", "-o", out]) == 0
    doc = json.load(open(out + ".json"))
    assert doc["signatures"][1]["Sketch"] == {"ksize": 21, "md5sum": hashlib.md5(b"\xff" * 128).hexdigest(),
                                              "mins": [2 ** 64 - 1] * 16, "num": 16}
    bad = str(tmp_path / "b")
    assert main(["sketch", "-f", fq, "-s", "16", "--kmv", "--khf", "-o", bad]) == 1
    assert not os.path.exists(bad + ".json")


def test_cpp_boss_collects_both_sketches(tmp_path, fq_reads):
    exe = str(tmp_path / "minhash_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "minhash_driver.cpp"), "-o", exe,
           "-L", LIBDIR, "-lhulkhip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    txt = tmp_path / "reads.txt"
    txt.write_bytes(b"\n".join(fq_reads) + b"\n")
    for k, S, interval in ((21, 50, 250), (31, 128, 0)):
        p = subprocess.run([exe, str(txt), str(k), str(W), str(S), str(interval)], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        doc = json.loads(p.stdout.strip().splitlines()[-1])
        vals = fed_values(*pack_reads(fq_reads), k)
        assert doc["n_seqs"] == 1000 and doc["n_minimizers"] == len(vals)
        assert doc["kmv"] == kmv_reference(vals, S).tolist() and doc["khf"] == khf_reference(vals, S).tolist()
    p = subprocess.run([exe, "noflag"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "-34|call not valid in this state: the context was created without HULK_FLAG_KMV", p.stdout + p.stderr
