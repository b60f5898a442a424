"""The KMV and KHF feeds on the GPU at the sizes where their code changes: every step of k_mh_scan's dispatch on S (NS = 1 .. 64 slots a
lane) and the size above it, the cap of 4096 values (64 blocks of kmv_insert_wave), and the line 2k + 8 + ceil(log2 S) = 64 between
the min-reduction and the brute-force KHF feed.

Inputs, yardstick and the conditions that make the inputs a test: tests/minhash_inputs.py (the conditions run without a GPU in
tests/test_minhash_cpu.py).  Every comparison is array_equal.  The contexts are created with 4096 bins: the MinHash sketches do not
depend on the spectrum's size, the CWS tables of a context (S x bins) do."""
import numpy as np
import pytest

import minhash_inputs as mi
from conftest import pack_reads

pytestmark = pytest.mark.gpu


def sketcher(k, S, w=mi.W, flags=None):
    import hulk_amd
    from hulk_amd import _lib
    return hulk_amd.GpuSketcher(k, w, S, num_bins=mi.NUM_BINS, flags=_lib.HULK_FLAG_KMV | _lib.HULK_FLAG_KHF if flags is None else flags)


def got_minhash(g):
    from hulk_amd import _lib
    kmv, fed = g.minhash(_lib.HULK_MINHASH_KMV)
    khf, fed2 = g.minhash(_lib.HULK_MINHASH_KHF)
    assert fed == fed2 == g.counters()["n_minimizers"]
    return kmv, khf, fed


def assert_minhash(g, want, n_fed, S, what):
    """want: (KMV, KHF) of the reference at size S"""
    kmv, khf, fed = got_minhash(g)
    want_kmv, want_khf = want
    assert fed == n_fed, f"{what}: {fed} values fed, want {n_fed}"
    assert len(kmv) == min(S, n_fed) == len(want_kmv), f"{what}: {len(kmv)} KMV entries"
    bad = np.nonzero(kmv != want_kmv)[0]
    assert len(bad) == 0, f"{what}: KMV differs in {len(bad)} of {len(kmv)} entries, first at {bad[0]}: got {kmv[bad[0]]}, want {want_kmv[bad[0]]}"
    bad = np.nonzero(khf != want_khf)[0]
    assert len(khf) == S and len(bad) == 0, (f"{what}: KHF differs in {len(bad)} of {S} slots, first at {bad[0]}, last at {bad[-1]}: got {khf[bad[0]]}, "
                                             f"want {want_khf[bad[0]]}; {int((khf[bad] == mi.U64_MAX).sum())} of them are MaxUint64")


# ---- 1. every step of the dispatch, every binning path -----------------------------------------------------------------------------
@pytest.mark.parametrize("S", mi.DISPATCH_SIZES)
@pytest.mark.parametrize("k", [31, 21])
def test_every_size_of_the_dispatch_on_every_path(k, S):
    """k = 31: brute force, k_mh_scan<NS> with NS = 1, 2, 4, .. 64 as S grows (the list and the table) and mh_feed_wave's slot loop (the
    generic kernel); one size above a step the top lanes own slots behind S.  k = 21: the min-reduction at every size.  Each path alone
    and the three in one context"""
    paths = mi.path_inputs(k)
    g_all = sketcher(k, S)
    for name in mi.PATHS:
        bases, offsets, vals = paths[name]
        g = sketcher(k, S)
        g.add_reads(bases, offsets)
        assert_minhash(g, mi.sliced(mi.path_reference(k, name), S), len(vals), S, f"k {k} S {S} {name}")
        g.close()
        g_all.add_reads(bases, offsets)
    assert_minhash(g_all, mi.sliced(mi.path_reference(k, "all"), S), len(paths["all"][2]), S, f"k {k} S {S} all paths in one context")
    g_all.finish()
    assert_minhash(g_all, mi.sliced(mi.path_reference(k, "all"), S), len(paths["all"][2]), S, f"k {k} S {S} after finish")
    g_all.close()


# ---- 2. KMV at the cap ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", mi.CAP_SIZES)
@pytest.mark.parametrize("k", [31, 21])
def test_kmv_at_the_cap(k, S):
    """fewer values than S (the tail stays MaxUint64 and is not returned), more values than S, and every value twice: at S = 4095 the
    bound lies between the two copies of one value"""
    for name in mi.CAP_STREAMS:
        calls, vals = mi.cap_stream(k, name)
        g = sketcher(k, S)
        for bases, offsets in calls:
            g.add_reads(bases, offsets)
        want = (mi.kmv_reference(vals, S), mi.sliced(mi.path_reference(k, "list"), S)[1] if name != "fewer" else mi.khf_reference(vals, S, chunk=1 << 11))
        assert_minhash(g, want, len(vals), S, f"k {k} S {S} {name}")
        if name == "twice" and S == 4095:
            assert got_minhash(g)[0][S - 1] == np.sort(vals)[S], "the slot at the bound"
        g.close()


# ---- 3. the order of the reads ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", mi.ORDER_SIZES)
def test_the_order_of_the_reads_does_not_matter(S):
    """descending by the reads' smallest minimizer: once the sketch is full every read's smallest value enters at rank 0 and carries
    an entry through all S / 64 blocks of kmv_insert_wave (64 of them at S = 4096), and the bound falls read after read"""
    k = 31
    want = mi.sliced(mi.path_reference(k, "list"), S)
    n = len(mi.path_inputs(k)["list"][2])
    for order in mi.ORDERS:
        reads = mi.ordered_reads(k, order)
        g = sketcher(k, S)
        for a in range(0, len(reads), 50):                          # eight calls: the bound of a call is what the calls before left
            g.add_reads(*pack_reads(reads[a:a + 50]))
        assert_minhash(g, want, n, S, f"k {k} S {S} reads {order}")
        g.close()


# ---- 4. merge at the cap ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 31])
def test_merge_of_two_halves_at_the_cap(k):
    """hulk_minhash_merge of both kinds at S = 4096: k = 21 a context that feeds by the min-reduction, k = 31 a brute-force one"""
    from hulk_amd import _lib
    S = mi.CAP
    reads = mi.path_reads()["list"] + mi.path_reads()["generic"]
    half = len(mi.path_reads()["list"]) // 2
    a, b = sketcher(k, S), sketcher(k, S)
    a.add_reads(*pack_reads(reads[:half]))
    b.add_reads(*pack_reads(reads[half:]))
    fed_a = got_minhash(a)[2]
    vals = np.concatenate([mi.path_inputs(k)["list"][2], mi.path_inputs(k)["generic"][2]])
    assert fed_a + got_minhash(b)[2] == len(vals) and len(got_minhash(a)[0]) == S == len(got_minhash(b)[0])
    for algo in (_lib.HULK_MINHASH_KMV, _lib.HULK_MINHASH_KHF):
        a.minhash_merge(algo, b.minhash(algo)[0])
    assert_minhash(a, (mi.kmv_reference(vals, S), mi.khf_reference(vals, S, chunk=1 << 11)), fed_a, S, f"k {k} merged halves at S {S}")
    for g in (a, b):
        g.close()


# ---- 5. the line between the two KHF feeds ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,S", [(k, S) for k in sorted(mi.BOUNDARY_S_LO) for S in mi.boundary_sizes(k)])
def test_the_line_between_the_two_khf_feeds(k, S):
    """w = 1, values up to 2^(2k + 8).  S_lo = 2^(64 - 2k - 8): the last size of the min-reduction; S_lo + 1: the first brute-force
    size, the last slot wraps; 2 * S_lo - 1 and 2 * S_lo: at least a quarter of the slots above S_lo wrap.  A feed on the wrong
    side of the line gives (i + 1) * min(x) there.  (At 2 * S_lo, a power of two, floor and ceiling of log2 S are the same number: it
    is S_lo + 1 and 2 * S_lo - 1 that tell the two apart.)"""
    bases, offsets, vals = mi.boundary_input(k)
    want = (mi.kmv_reference(vals, S), mi.khf_reference(vals, S))
    naive = mi.khf_naive(vals, S)
    print(f"k {k} S {S} (S_lo {mi.BOUNDARY_S_LO[k]}): {int((want[1] != naive).sum())} slots of the reference differ from (i+1) * min(x)")
    g = sketcher(k, S, w=mi.BOUNDARY_W)
    g.add_reads(bases, offsets)
    assert_minhash(g, want, len(vals), S, f"k {k} w 1 S {S} (S_lo {mi.BOUNDARY_S_LO[k]})")
    g.close()
