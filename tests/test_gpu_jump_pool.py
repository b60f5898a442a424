"""The register pool of k_jump_bin (hulk_spectrum.hip): the chains a round of 64 values leaves unfinished are handed to a pool of
the wave with ds_permute_b32, run again in dense pool rounds and drained after the wave's last region.

Every setting of the profiling build (HULK_JUMP_CUT / HULK_JUMP_PCUT / HULK_JUMP_REGIONS, HULK_JUMP_C) runs all cases in one
subprocess, with HULK_POISON=0xff.  The poison fills ml.key when the list is allocated, not before every batch: in the cases of
one batch a chain that is never stored leaves a key of 0xffffffff, which no spectrum counts, so it shows up as a lost increment
(`hist.sum() == n_minimizers`).  In the cases of several batches (ring_wraps, fill_nonzero) such a chain would leave the key an
earlier batch wrote there, a wrong increment rather than a lost one; those cases rest on the comparison with the oracle alone.
Each result is compared with the CPU oracle (spectrum, minimizer count, count-min counters and `mins` bit-exact, weights to
1e-9), and a case's spectrum must be byte-identical across all settings."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import pack_reads
from oracle import pyorc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP_LIB = os.path.join(ROOT, "hulk_amd", "csrc", "libhulkhip_exp.so")
WEIGHT_RTOL = 1e-9
S = 16
SWITCHES = ("HULK_JUMP_CUT", "HULK_JUMP_PCUT", "HULK_JUMP_REGIONS", "HULK_JUMP_C", "HULK_POISON")


def random_reads(seed, n, length=150):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [bytes(acgt[rng.integers(0, 4, size=length)]) for _ in range(n)]


def _cases():
    """name -> (k, interval, batch, reads, cuts of the host calls); a region is 16 reads, ~432 values at w = 9"""
    c = {}
    # one read, ~27 values in a single round: at cut 63 that is fewer values than cut and every chain goes through the pool and
    # the drain; at the default cut of 24 the round ends with a few chains live and only those are pooled and drained
    c["reads_1"] = (21, 0, 0, random_reads(11, 1), [0, 1])
    c["reads_16"] = (21, 0, 0, random_reads(12, 16), [0, 16])         # one region, 7 rounds: the pool fills, wraps, is re-compacted
    c["reads_17"] = (21, 0, 0, random_reads(13, 17), [0, 17])         # a region with one read; a last wave with fewer than R regions
    c["reads_33"] = (21, 0, 0, random_reads(14, 33), [0, 33])
    big = random_reads(3, 3000)                                       # one spectrum, ~80 k values: chains beyond 25 steps occur
    c["one_spectrum"] = (21, 0, 0, big, [0, 3000])
    ring = random_reads(7, 7000)                                      # interval 1000 is no multiple of 16: regions straddle spectra and
    c["ring_wraps"] = (21, 1000, 3, ring, [0, 7000])                  # the ring of 3 + 1 wraps: a pool holds entries of several slots
    c["fill_nonzero"] = (21, 1000, 3, ring, [0, 700, 7000])           # calls cut at 700: P.fill != 0
    for k in (15, 22, 23, 31):
        c[f"k{k}"] = (k, 0, 0, big[:1500], [0, 1500])
    return c


CASES = _cases()
SETTINGS = {
    "default": {},
    "cut1_pcut1": {"HULK_JUMP_CUT": "1", "HULK_JUMP_PCUT": "1"},       # single-chain hand-overs: the pool reaches exactly 64
    "cut63_pcut1": {"HULK_JUMP_CUT": "63", "HULK_JUMP_PCUT": "1"},     # nearly every chain through the pool; cut + pcut = 64
    "cut32_pcut32": {"HULK_JUMP_CUT": "32", "HULK_JUMP_PCUT": "32"},
    "regions_1": {"HULK_JUMP_REGIONS": "1"},
    "regions_3": {"HULK_JUMP_REGIONS": "3"},                           # the region count is no multiple of it
    "regions_8": {"HULK_JUMP_REGIONS": "8"},
    "cut0": {"HULK_JUMP_CUT": "0"},                                    # comparators: every round runs to its end, no pool
    "plain_c": {"HULK_JUMP_C": "1"},
}

_RUNNER = """
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
import hulk_amd
from hulk_amd import _lib
assert _lib.load().hulk_build_info().endswith(b" experiments=1")
for name, k, interval, batch, cuts in json.loads(sys.argv[2]):
    d = np.load(sys.argv[1] + "/" + name + ".npz")
    g = hulk_amd.GpuSketcher(k, 9, {S}, interval, batch=batch)
    for a, b in zip(cuts[:-1], cuts[1:]):
        g.add_reads(d["bases"], d["offsets"][a:b + 1])
    hist, err = g.histogram(), ""
    try:
        g.finish()
    except hulk_amd.HulkError as e:
        err = str(e)
    mins, weights = g.sketch() if not err else (np.zeros(0), np.zeros(0))
    np.savez(sys.argv[3] + "/" + name + ".npz", hist=hist, cms=g.cms() if not err else np.zeros(0), mins=mins, weights=weights,
             n_min=np.uint64(g.counters()["n_minimizers"]), err=np.array(err))
    g.close()
print("DONE", flush=True)
"""


@pytest.fixture(scope="module")
def gpu_runs(tmp_path_factory):
    """{setting: {case: arrays}}: all cases through the profiling build, one subprocess per setting"""
    assert os.path.exists(EXP_LIB), "profiling build (libhulkhip_exp.so) not built"
    d_in = tmp_path_factory.mktemp("pool_in")
    for name, (k, interval, batch, seqs, cuts) in CASES.items():
        bases, offsets = pack_reads(seqs)
        np.savez(str(d_in / f"{name}.npz"), bases=bases, offsets=offsets)
    env0 = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    spec = json.dumps([[n, c[0], c[1], c[2], c[4]] for n, c in CASES.items()])
    out = {}
    for setting, env in SETTINGS.items():
        d_out = tmp_path_factory.mktemp("pool_" + setting)
        r = subprocess.run([sys.executable, "-c", _RUNNER.format(root=ROOT, S=S), str(d_in), spec, str(d_out)],
                           env=dict(env0, HULK_LIB="exp", HULK_POISON="0xff", **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "DONE" in r.stdout, f"{setting}: {r.stderr[-2000:]}"
        out[setting] = {n: dict(np.load(str(d_out / f"{n}.npz"))) for n in CASES}
    return out


_ORACLE = {}


def oracle(name):
    """the CPU oracle's result of a case (computed once)"""
    if name not in _ORACLE:
        k, interval, batch, seqs, cuts = CASES[name]
        o = pyorc.Sketcher(k, 9, S, 0, 1.0, interval)
        o.add_reads(*pack_reads(seqs))
        hist, err = o.histogram().astype(np.uint32), ""
        try:
            o.finish()
        except pyorc.OracleError as e:
            err = str(e)
        mins, weights = o.sketch()
        _ORACLE[name] = dict(hist=hist, cms=o.cms(), mins=mins, weights=weights, n_min=o.counters()["n_minimizers"], err=err)
        o.close()
    return _ORACLE[name]


def assert_matches_oracle(got, name):
    want = oracle(name)
    assert int(got["n_min"]) == want["n_min"]
    assert np.array_equal(got["hist"], want["hist"]), f"{int((got['hist'] != want['hist']).sum())} bins differ"
    if CASES[name][1] == 0:
        assert int(got["hist"].sum(dtype=np.uint64)) == want["n_min"], "spectrum increments lost"
    # (a spectrum with under 1 % of its bins used is fatal at finish in the reference, "not used yet": the cases of a few reads
    #  end there, on both sides, and have a spectrum but no sketch)
    assert (want["err"] in str(got["err"])) if want["err"] else not str(got["err"]), (str(got["err"]), want["err"])
    if want["err"]:
        return
    assert np.array_equal(got["cms"], want["cms"]), "count-min counters differ"
    assert np.array_equal(got["mins"], want["mins"]), f"{int((got['mins'] != want['mins']).sum())} of {S} mins differ"
    assert np.allclose(got["weights"], want["weights"], rtol=WEIGHT_RTOL, atol=0)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_pooled_jump_matches_the_oracle(gpu_runs, setting, name):
    assert_matches_oracle(gpu_runs[setting][name], name)


@pytest.mark.parametrize("name", list(CASES))
def test_spectrum_is_identical_across_settings(gpu_runs, name):
    want = gpu_runs["default"][name]["hist"]
    for setting in SETTINGS:
        got = gpu_runs[setting][name]["hist"]
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), setting
