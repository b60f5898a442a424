"""The MinHash side of the ABI without a GPU: the header and the binding agree on the two flags and the two entry points, the
numpy restatement of minhash.KMVsketch / KHFsketch (src/minhash/kmv.go:39-71, khf.go:34-45) that tests/test_gpu_minhash.py
compares the GPU with behaves as the reference does on hand cases, and a HULKdata with real kmv + khf signatures round-trips
through both loaders; and the inputs of tests/test_gpu_minhash_sizes.py exercise what they claim (the check_* functions of
tests/minhash_inputs.py, on the reference alone)."""
import ctypes
import os
import re

import numpy as np
import pytest

# the reference, restated, lives in tests/minhash_inputs.py (the GPU test modules import that ONE definition, from here or there)
import minhash_inputs as mi
from conftest import ROOT
from minhash_inputs import U64_MAX, khf_merge_reference, khf_reference, kmv_reference  # noqa: F401


def test_header_and_binding_agree_on_the_minhash_abi():
    from hulk_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hulk_hip.h")).read()
    defs = dict(re.findall(r"^#define (HULK_\w+) (\d+)u?\b", hdr, re.M))
    assert int(defs["HULK_FLAG_KMV"]) == 128 == _lib.HULK_FLAG_KMV
    assert int(defs["HULK_FLAG_KHF"]) == 256 == _lib.HULK_FLAG_KHF
    assert int(defs["HULK_MINHASH_KMV"]) == 0 == _lib.HULK_MINHASH_KMV
    assert int(defs["HULK_MINHASH_KHF"]) == 1 == _lib.HULK_MINHASH_KHF
    assert int(defs["HULK_MINHASH_MAX_SKETCH"]) == _lib.HULK_MINHASH_MAX_SKETCH >= 4096
    assert int(defs["HULK_ABI_VERSION"]) == 4 == _lib.HULK_ABI_VERSION
    for sym in ("hulk_get_minhash", "hulk_minhash_merge"):
        assert re.search(r"^int %s\(hulk_ctx \*ctx, int algo, " % sym, hdr, re.M), sym
        assert sym in _lib.ABI_SYMBOLS
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "hulk_get_minhash") and hasattr(L, "hulk_minhash_merge")
    # 1 << 9 is still no flag: every defined flag bit lies below it
    flags = [int(v) for k, v in defs.items() if k.startswith("HULK_FLAG_")]
    assert sorted(flags) == [1 << i for i in range(9)]


def test_unknown_flag_is_still_refused_before_any_device_is_touched():
    """hulk_create checks the flags before it looks for a device: 1 << 9 is refused with the text it always had, here too."""
    from hulk_amd import _lib
    L = _lib.load()
    p = _lib.HulkParams(k=21, w=9, sketch_size=8, decay_ratio=1.0, flags=1 << 9)
    ctx = ctypes.c_void_p()
    assert L.hulk_create(ctypes.byref(p), ctypes.byref(ctx)) == -30
    assert L.hulk_last_error(None).endswith(b"unknown flags")
    # the documented cap of a MinHash context, also checked in front of the device
    for flag in (_lib.HULK_FLAG_KMV, _lib.HULK_FLAG_KHF):
        for size in (0, _lib.HULK_MINHASH_MAX_SKETCH + 1):
            p = _lib.HulkParams(k=21, w=9, sketch_size=size, decay_ratio=1.0, flags=flag)
            assert L.hulk_create(ctypes.byref(p), ctypes.byref(ctx)) == -30
            assert b"sketch_size <= 4096" in L.hulk_last_error(None)


def test_kmv_restatement_keeps_duplicates_and_short_streams():
    # duplicates are kept: the heap never de-duplicates (kmv.go:41-52 is a TODO)
    assert kmv_reference([9, 3, 7, 3, 3, 8, 1], 4).tolist() == [1, 3, 3, 3]
    assert kmv_reference([5, 5, 5, 5], 2).tolist() == [5, 5]
    # fewer values than sketch_size: all of them, ascending
    assert kmv_reference([4, 2, 2], 8).tolist() == [2, 2, 4]
    assert kmv_reference([], 8).tolist() == []
    # ... and the literal heap of kmv.go:39-71 gives the same multiset
    import heapq
    rng = np.random.default_rng(5)
    vals = rng.integers(0, 40, size=300).astype(np.uint64)
    heap = []
    for v in vals.tolist():
        if len(heap) < 16:
            heapq.heappush(heap, -v)
        elif v < -heap[0]:
            heapq.heapreplace(heap, -v)
    assert sorted(-x for x in heap) == kmv_reference(vals, 16).tolist()


def test_khf_restatement_wraps_like_uint64():
    assert khf_reference([], 3).tolist() == [U64_MAX] * 3
    assert khf_reference([10, 7], 4).tolist() == [7, 14, 21, 28]
    x = (1 << 63) + 5                                        # >= 2^63: slot 1 wraps (2x mod 2^64 = 10), slot 2 does not fall below
    got = khf_reference([x], 4).tolist()
    assert got == [x, 10, (3 * x) % (1 << 64), 20]
    # a larger value wins a slot through the wrap: min over x of (i+1)x is NOT (i+1) min(x) there
    got = khf_reference([100, x], 4).tolist()
    assert got == [100, 10, 300, 20]
    want = [min(((i + 1) * v) % (1 << 64) for v in (100, x, 12345678901234567)) for i in range(64)]
    assert khf_reference([100, x, 12345678901234567], 64).tolist() == want
    assert khf_merge_reference([1, 9, U64_MAX], [4, 2, 7]).tolist() == [1, 2, 7]


def test_minhash_signatures_round_trip_through_both_loaders(tmp_path):
    from hulk_amd import smash as smash_mod
    from hulk_amd.sketchio import HULKdata, HistoSketch, KHFSketch, KMVSketch, load_hulk_data, md5sum
    rng = np.random.default_rng(11)
    files, kmvs, khfs = [], [], []
    for i in range(3):
        vals = rng.integers(0, 1 << 62, size=400, dtype=np.uint64) | np.uint64(1 << 63 if i == 2 else 0)
        kmv, khf = kmv_reference(vals, 32), khf_reference(vals, 32)
        d = HULKdata()
        d.add(HistoSketch(27, rng.integers(0, 1 << 40, size=32, dtype=np.uint64), rng.random(32), 27 ** 4, False))
        d.add(KMVSketch(27, len(kmv), kmv))
        d.add(KHFSketch(27, 32, khf))
        d.filename, d.banner_label = f"r{i}.fq,", "blank"
        p = str(tmp_path / f"s{i}.json")
        d.write_json(p)
        files.append(p); kmvs.append(kmv); khfs.append(khf)
        back = load_hulk_data(p)                              # (verifies every MD5)
        assert [a for a, _ in back.signatures] == ["histosketch", "kmv", "khf"]
        assert np.array_equal(back.signatures[1][1].mins, kmv) and back.signatures[1][1].num == 32
        assert np.array_equal(back.signatures[2][1].mins, khf)
        assert back.signatures[1][1].md5sum == md5sum(kmv)
    for algo, want in (("kmv", kmvs), ("khf", khfs)):
        order, mins, weights, _ = smash_mod.load_sketches(files, 27, algo)
        assert order == sorted(files) and mins.shape == (3, 32)
        assert np.array_equal(mins, np.stack(want)) and not weights.any()


# ---- the inputs of tests/test_gpu_minhash_sizes.py are a test (conditions on the reference alone) -----------------------------------
@pytest.mark.parametrize("k", [21, 31])
def test_the_path_inputs_feed_every_path_and_fill_the_largest_sketch(k):
    mi.check_path_inputs(k)


def test_at_k_31_the_wrap_decides_more_than_half_of_the_slots_of_every_size():
    mi.check_wrap_decides(31)
    mi.check_no_wrap(21)
    assert set(mi.DISPATCH_SIZES) >= {64 * ns + d for ns in (1, 2, 4, 8, 16, 32) for d in (0, 1)} | {4095, 4096}


@pytest.mark.parametrize("k", [21, 31])
def test_kmv_streams_at_the_cap_and_the_bound_between_two_copies(k):
    mi.check_cap_streams(k)


@pytest.mark.parametrize("k", [21, 31])
def test_descending_reads_make_the_bound_fall_in_half_of_the_reads(k):
    mi.check_orders(k)


@pytest.mark.parametrize("k", sorted(mi.BOUNDARY_S_LO))
def test_the_inputs_show_the_line_between_the_two_khf_feeds(k):
    wrapped = mi.check_boundary(k)
    print(f"k {k}: S_lo {mi.BOUNDARY_S_LO[k]}, seed {mi.BOUNDARY_SEEDS[k]}, {wrapped} slots above S_lo wrap at 2 * S_lo; sizes {mi.boundary_sizes(k)}")
    assert 2 * k + 8 + (mi.BOUNDARY_S_LO[k] - 1).bit_length() == 64 and mi.BOUNDARY_S_LO[k] in mi.boundary_sizes(k)
