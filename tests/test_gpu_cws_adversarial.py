"""The CWS resolve at ties, near-ties and pruning margins, on the device, against the CPU oracle.

The inputs are the seeded scenarios of tests/cws_adversarial.py; tests/test_cws_adversarial_cpu.py certifies them (planted gaps at
50 digits, class separation, more than 64 tied wave tiles, drift sensitivity) and checks the oracle against a numpy replay.
Here the same scenarios run through libhulkhip with external tables (hulk_set_cws_tables):
  1. single flushes (hulk_add_histogram + hulk_flush): near-ties below fp32 resolution, exact ties over 2 ... 190 wave tiles (the
     nc > 64 branches of k_cws_resolve), a row with every K >= 0, A == 0, ties across a tile border, between the last, partly
     filled tile and tile 0, and at one position of three tiles — merged resolve and, with snapshots, the per-interval resolve + k_cws_apply_snap;
  2. later flushes at the weight's margin, pruning on / HULK_FLAG_NO_SKIP / HULK_FLAG_NO_PRUNE, bitwise equal among themselves,
     once with all gaps and once with every row of both slot groups needing the band of k_scan_test;
  3. multi-interval batches from reads (batch 1, 3, 16; one and two work lanes; snapshots; a slot shard; HULK_FLAG_CMS_CHAIN);
  4. concept drift (k_cws_resolve_drift), every per-interval snapshot.
Bar: `mins` equal to the oracle's, `weights` within 1e-9 relative (1e-7 with decay), count-min counters as in test_gpu_parity.py.
The two-rank hulk_step_sharded_host path is not run here: the worker of tests/test_gpu_two_rank.py builds its own contexts with
generated tables and cannot take external ones without being copied.

33 tests, about 60 contexts of 16 slots x 50625 bins (20 MB of tables each); on an MI355X the file takes 3 s (the slowest test,
with its generator, 0.6 s).
"""
import numpy as np
import pytest

import cws_adversarial as adv

pytestmark = pytest.mark.gpu

WEIGHT_RTOL = 1e-9
DRIFT_RTOL = 1e-7
_cache = {}


def oracle(sc):
    if sc.name not in _cache:
        _cache[sc.name] = adv.oracle_states(sc) + (oracle_cms(sc),)
    return _cache[sc.name]


def oracle_cms(sc):
    from oracle import pyorc
    o = pyorc.Sketcher(adv.K, adv.W, 1, adv.B, sc.decay, sc.interval)
    adv._feed(o, sc.spectra, sc.reads, sc.interval, sc.n_int, lambda _o: None)
    c = o.cms(); o.close()
    return c


def batch_one(sc, **kw):
    """the library at batch = 1 (one interval per flush): what every other batching must reproduce bit for bit"""
    key = (sc.name, "batch1", tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = adv.gpu_states(sc, batch=1, **kw)
    return _cache[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_oracle(sc, gm, gw, om, ow, what=""):
    rtol = WEIGHT_RTOL if sc.decay == 1.0 else DRIFT_RTOL
    assert gm.shape == om.shape
    bad = np.argwhere(gm != om)
    assert not len(bad), f"{sc.name} {what}: mins differ from the oracle at (flush, slot) {bad.tolist()[:12]}: device {gm[gm != om][:12]}, oracle {om[gm != om][:12]}"
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ow == 0, np.abs(gw), np.abs(gw - ow) / np.abs(ow))
    print(f"{sc.name} {what}: largest relative weight error {rel.max():.3e}")
    assert np.allclose(gw, ow, rtol=rtol, atol=0), f"{sc.name} {what}: weights"


def assert_bitwise(am, aw, bm, bw, what):
    assert np.array_equal(am, bm), f"{what}: mins differ at {np.argwhere(am != bm).tolist()[:12]}"
    assert np.array_equal(bits(aw), bits(bw)), f"{what}: weights differ at {np.argwhere(bits(aw) != bits(bw)).tolist()[:12]}"


def assert_cms(sc, cms, ocms):
    if sc.decay == 1.0:
        assert np.array_equal(cms, ocms)
    else:
        assert np.allclose(cms, ocms, rtol=1e-9, atol=1e-300)


# ---- 1. single flushes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", [adv.near_ties_single, adv.quantised_single], ids=["near_ties", "quantised"])
def test_single_flush(gen):
    sc = gen()
    om, ow, ocms = oracle(sc)
    gm, gw, _, cms = adv.gpu_states(sc)                            # k_cws_resolve<true> + k_cws_apply
    assert_oracle(sc, gm, gw, om, ow, "merged")
    assert_cms(sc, cms, ocms)
    sm, sw, _, _ = adv.gpu_states(sc, snapshots=1)                 # k_cws_resolve<false> + k_cws_apply_snap
    assert_oracle(sc, sm, sw, om, ow, "per interval")
    assert_bitwise(sm, sw, gm, gw, f"{sc.name}: per-interval against merged resolve")
    for (t, s), x in sc.winners.items():
        assert gm[t, s] == x


def test_single_flush_without_pruning_reads_the_same():
    from hulk_amd import _lib
    sc = adv.quantised_single()
    a = adv.gpu_states(sc)
    b = adv.gpu_states(sc, flags=_lib.HULK_FLAG_NO_PRUNE)
    assert_bitwise(a[0], a[1], b[0], b[1], "quantised_single: HULK_FLAG_NO_PRUNE")


# ---- 2. later flushes at the weight's margin -------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", [adv.margins, adv.scan_margin], ids=["margins", "scan_margin"])
def test_margins_with_and_without_pruning(gen):
    """margins: both signs of every gap, the duplicate, one gap outside the band.  scan_margin: in every row of both slot groups
    the fp32 bound k_scan_test forms for z's tile lies above the weight (certified on the CPU), so only the band has it read."""
    from hulk_amd import _lib
    sc = gen()
    om, ow, ocms = oracle(sc)
    res = {}
    for name, flags in (("prune", 0), ("no_skip", _lib.HULK_FLAG_NO_SKIP), ("no_prune", _lib.HULK_FLAG_NO_PRUNE)):
        res[name] = adv.gpu_states(sc, flags=flags)
        assert_oracle(sc, res[name][0], res[name][1], om, ow, name)
        assert_cms(sc, res[name][3], ocms)
    for name in ("no_skip", "no_prune"):
        assert_bitwise(res[name][0], res[name][1], res["prune"][0], res["prune"][1], f"{sc.name}: {name} against pruning on")
    for (t, s), x in sc.winners.items():
        assert res["prune"][0][t, s] == x, (t, s)
    # the quiet flushes 1..3 were pruned, the late one was not passed over
    for name in ("prune", "no_skip"):
        st = res[name][2]
        quiet_read, quiet_all = st[3][0] - st[0][0], st[3][1] - st[0][1]
        print(f"{sc.name} {name}: tiles read in flushes 1-3: {quiet_read} of {quiet_all}; in flush 4: {st[4][0] - st[3][0]}")
        assert quiet_read <= 0.05 * quiet_all
        assert 0 < st[4][0] - st[3][0] <= 0.05 * (st[4][1] - st[3][1])
    st = res["no_prune"][2]
    assert st[4][0] == st[4][1]
    snap = adv.gpu_states(sc, snapshots=1)                         # the same margins through k_cws_apply_snap
    assert_bitwise(snap[0], snap[1], res["prune"][0], res["prune"][1], f"{sc.name}: snapshot context")


# ---- 3. multi-interval batches from reads ----------------------------------------------------------------------------------------
READS = {"near_ties": adv.batches_from_reads, "quantised": adv.quantised_from_reads}


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("batch", [1, 3, 16])
@pytest.mark.parametrize("which", ["near_ties", "quantised"])
def test_batches_from_reads(which, batch, lanes):
    sc = READS[which]()
    om, ow, ocms = oracle(sc)
    gm, gw, _, cms = adv.gpu_states(sc, batch=batch, work_lanes=lanes)
    assert_oracle(sc, gm, gw, om[-1:], ow[-1:], f"batch {batch} lanes {lanes}")
    assert_cms(sc, cms, ocms)
    bm, bw, _, _ = batch_one(sc)
    assert_bitwise(gm, gw, bm, bw, f"{sc.name}: batch {batch} lanes {lanes} against batch 1")
    # (quantised_from_reads designs no winners: that the earliest (interval, bin) of the tie wins is the oracle comparison above,
    # and test_quantised_tables_from_reads asserts on the CPU that the oracle's min is the smallest tied bin of interval 0)
    for (t, s), x in sc.winners.items():
        assert gm[0, s] == x


@pytest.mark.parametrize("batch", [1, 3, 16])
@pytest.mark.parametrize("which", ["near_ties", "quantised"])
def test_batches_from_reads_every_snapshot(which, batch):
    sc = READS[which]()
    om, ow, _ = oracle(sc)
    gm, gw, _, _ = adv.gpu_states(sc, batch=batch, snapshots=1)
    assert_oracle(sc, gm, gw, om, ow, f"snapshots, batch {batch}")
    bm, bw, _, _ = batch_one(sc, snapshots=1)
    assert_bitwise(gm, gw, bm, bw, f"{sc.name}: snapshots of batch {batch} against batch 1")
    fm, fw, _, _ = batch_one(sc)
    assert_bitwise(gm[-1:], gw[-1:], fm, fw, f"{sc.name}: last snapshot against the merged resolve")


@pytest.mark.parametrize("which", ["near_ties", "quantised"])
def test_slot_shard_against_the_full_tables(which):
    sc = READS[which]()
    om, ow, _ = oracle(sc)
    lo, n = 3, 9                                                   # slots 3..11: both 8-slot groups of the full run are cut
    gm, gw, _, _ = adv.gpu_states(sc, batch=3, slot_begin=lo, slot_count=n)
    bm, bw, _, _ = batch_one(sc)
    assert_bitwise(gm[:, lo:lo + n], gw[:, lo:lo + n], bm[:, lo:lo + n], bw[:, lo:lo + n], f"{sc.name}: slot shard")
    assert np.array_equal(gm[0, lo:lo + n], om[-1, lo:lo + n])
    other = np.r_[0:lo, lo + n:sc.S]
    assert (gm[0, other] == 0).all() and (gw[0, other] == adv.MAXF).all()


def test_forced_chain_fallback_of_the_count_min():
    from hulk_amd import _lib
    sc = adv.batches_from_reads()
    om, ow, ocms = oracle(sc)
    gm, gw, _, cms = adv.gpu_states(sc, batch=3, flags=_lib.HULK_FLAG_CMS_CHAIN)
    assert_oracle(sc, gm, gw, om[-1:], ow[-1:], "HULK_FLAG_CMS_CHAIN")
    assert_cms(sc, cms, ocms)
    bm, bw, _, _ = batch_one(sc)
    assert_bitwise(gm, gw, bm, bw, "batches_from_reads: HULK_FLAG_CMS_CHAIN")


# ---- 4. concept drift --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3, 16])
@pytest.mark.parametrize("decay", [0.02, 0.5])
def test_drift_every_snapshot(decay, batch):
    sc = adv.drift(decay)
    om, ow, ocms = oracle(sc)
    gm, gw, _, cms = adv.gpu_states(sc, batch=batch, snapshots=1)
    assert_oracle(sc, gm, gw, om, ow, f"batch {batch}")
    assert_cms(sc, cms, ocms)
    bm, bw, _, _ = batch_one(sc, snapshots=1)
    assert_bitwise(gm, gw, bm, bw, f"{sc.name}: snapshots of batch {batch} against batch 1")
    for s, t, _p, x, d in sc.info["planted"]:
        assert (gm[t, s] == x) == (d > 0), (s, t, x, d)
    t0, z0, _z1 = sc.info["zero_pair"]                             # A == 0 == w / decayWeight: the strict < keeps the first
    assert gm[t0, 13] == z0 and gw[t0, 13] == 0.0
    if batch == 16:
        fm, fw, _, _ = adv.gpu_states(sc, batch=batch)             # without snapshots: the same final sketch
        assert_bitwise(fm, fw, gm[-1:], gw[-1:], f"{sc.name}: no snapshots")


# ---- 5. tables outside the domain of the fp32 screen ---------------------------------------------------------------------------------
def test_tables_whose_k_is_not_finite_in_fp32_are_refused():
    """K = c * exp(b - r) is what the scan orders tiles by, in fp32.  With K32 = -inf in a row the resolve's band
    (g + 1e-5 |g|) is NaN and finds no candidate; with +inf everywhere `g < INFINITY` is false: either way the slot silently
    keeps its old content where the oracle updates (read off the code; docs/EXPERIMENTS.md).  hulk_set_cws_tables
    now refuses such tables (HULK_ERR_ARG), over the rows the context owns; FLT_MAX itself is inside the domain."""
    import hulk_amd
    from hulk_amd import _lib
    k, S = 7, 8
    nb = k ** 4
    rng = np.random.default_rng(11)
    r = rng.gamma(2.0, 1.0, size=(S, nb)); c = np.log(rng.gamma(2.0, 1.0, size=(S, nb))); b = rng.random((S, nb)) * r
    hist = ((rng.random(nb) < 0.5) * rng.integers(1, 9, size=nb)).astype(np.uint32)
    hist[100] = 3
    fmax = float(np.finfo(np.float32).max)
    for bad in (-1e39, 1e39, -np.inf, np.inf, np.nan, np.nextafter(fmax, np.inf) * 1.0000001):
        g = hulk_amd.GpuSketcher(k, 3, S, num_bins=nb, cws_source=_lib.HULK_CWS_EXTERNAL)
        c2 = c.copy(); b2 = b.copy()
        c2[5, 100] = bad; b2[5, 100] = r[5, 100]                   # exp(b - r) == 1: K == c
        with pytest.raises(hulk_amd.HulkError, match="not finite in fp32") as e:
            g.set_cws_tables(r, c2, b2)
        assert e.value.code == -30                                  # HULK_ERR_ARG
        g.set_cws_tables(r, c, b)                                   # the context is still good for proper tables
        g.add_histogram(hist); g.flush()
        want = g.sketch()
        g.close()
    g = hulk_amd.GpuSketcher(k, 3, S, num_bins=nb, cws_source=_lib.HULK_CWS_EXTERNAL)
    c2 = c.copy(); b2 = b.copy()
    c2[5, 100] = -fmax; b2[5, 100] = r[5, 100]                     # -FLT_MAX: the largest magnitude inside the domain
    g.set_cws_tables(r, c2, b2)
    g.add_histogram(hist); g.flush()
    gm, gw = g.sketch(); g.close()
    assert gm[5] == 100 and np.array_equal(np.delete(gm, 5), np.delete(want[0], 5))
    g = hulk_amd.GpuSketcher(k, 3, S, num_bins=nb, cws_source=_lib.HULK_CWS_EXTERNAL, slot_begin=0, slot_count=4)
    c2[5, 100] = -np.inf
    g.set_cws_tables(r, c2, b2)                                    # row 5 is not this shard's: not looked at, not uploaded
    g.close()
