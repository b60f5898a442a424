"""The jump-hash step loop (jump_steps_asm in hulk_spectrum.hip) through k_jump_bin / k_jump_left and the 4-bit spectrum kernels.

A step of the loop turns key >> 33 into a double without a conversion (the shift result is the lower dword of a pair whose upper
dword is held at 0x43300000, one fma takes 2^52 + m to (m + 1) * 2^-31) and forms the upper dword of the LCG with chained
v_mad_u64_u32.  Every case runs on the profiling build in a subprocess (one process per setting, all cases of a setting in one):
the assembly loop with the default hand-over of slow chains, with none (HULK_JUMP_CUT=0) and the plain C++ loop (HULK_JUMP_C=1).
Each is compared with the CPU oracle: spectrum, minimizer count, count-min counters and `mins` bit-exact, weights to 1e-9."""
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


def random_reads(seed, n, length=150):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [bytes(acgt[rng.integers(0, 4, size=length)]) for _ in range(n)]


def _cases():
    """name -> (k, interval, batch, reads, cuts of the host calls)"""
    c = {}
    for n in (1, 15, 16, 17, 33):                         # empty waves, one region, a region edge (16 reads per region)
        c[f"reads_{n}"] = (21, 0, 0, random_reads(n, n), [0, n])
    ring = random_reads(7, 7000)                          # interval 1000 is no multiple of 16: regions straddle spectra; the ring of
    c["ring_wraps"] = (21, 1000, 3, ring, [0, 7000])      # 3 + 1 spectra wraps
    c["fill_nonzero"] = (21, 1000, 3, ring, [0, 700, 7000])
    big = random_reads(3, 3000)                           # one spectrum, ~80 k values: chains beyond 25 steps occur
    c["one_spectrum"] = (21, 0, 0, big, [0, 3000])
    c["copies"] = (21, 0, 0, random_reads(5, 1) * 2000, [0, 2000])      # 4-bit counters overflow -> nib_over -> exact recount
    c["copies_and_random"] = (21, 0, 0, random_reads(5, 1) * 2000 + big[:800], [0, 2800])   # ... with enough bins for a sketch
    c["k22"] = (22, 0, 0, big[:1500], [0, 1500])          # 234,256 bins: one range of 2^18
    c["k15"] = (15, 0, 0, big[:1500], [0, 1500])
    c["k23"] = (23, 0, 0, big[:1500], [0, 1500])          # 279,841 bins: two ranges of 2^18
    return c


CASES = _cases()
# the settings of the profiling build and the cases each runs
SETTINGS = {
    "asm": ({}, list(CASES)),
    "asm_cut0": ({"HULK_JUMP_CUT": "0"}, ["one_spectrum"]),
    "plain_c": ({"HULK_JUMP_C": "1"}, ["one_spectrum"]),
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
    """{setting: {case: arrays}}: every setting's cases through the profiling build, one subprocess per setting"""
    assert os.path.exists(EXP_LIB), "profiling build (libhulkhip_exp.so) not built"
    d_in = tmp_path_factory.mktemp("jump_in")
    for name, (k, interval, batch, seqs, cuts) in CASES.items():
        bases, offsets = pack_reads(seqs)
        np.savez(str(d_in / f"{name}.npz"), bases=bases, offsets=offsets)
    env0 = {k: v for k, v in os.environ.items() if k not in ("HULK_JUMP_CUT", "HULK_JUMP_C")}
    out = {}
    for setting, (env, names) in SETTINGS.items():
        d_out = tmp_path_factory.mktemp("jump_" + setting)
        spec = [[n, CASES[n][0], CASES[n][1], CASES[n][2], CASES[n][4]] for n in names]
        r = subprocess.run([sys.executable, "-c", _RUNNER.format(root=ROOT, S=S), str(d_in), json.dumps(spec), str(d_out)],
                           env=dict(env0, HULK_LIB="exp", **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "DONE" in r.stdout, f"{setting}: {r.stderr[-2000:]}"
        out[setting] = {n: dict(np.load(str(d_out / f"{n}.npz"))) for n in names}
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
    #  and the copies of one read end there, on both sides, and have a spectrum but no sketch)
    assert (want["err"] in str(got["err"])) if want["err"] else not str(got["err"]), (str(got["err"]), want["err"])
    if want["err"]:
        return
    assert np.array_equal(got["cms"], want["cms"]), "count-min counters differ"
    assert np.array_equal(got["mins"], want["mins"]), f"{int((got['mins'] != want['mins']).sum())} of {S} mins differ"
    assert np.allclose(got["weights"], want["weights"], rtol=WEIGHT_RTOL, atol=0)


@pytest.mark.parametrize("name", list(CASES))
def test_assembly_loop_matches_the_oracle(gpu_runs, name):
    """k_jump_bin hands the chains of a round's last <= 10 lanes to k_jump_left (the default)"""
    assert_matches_oracle(gpu_runs["asm"][name], name)


def test_assembly_loop_without_the_cut(gpu_runs):
    """HULK_JUMP_CUT=0: every round runs until its last chain is done, k_jump_left is not launched"""
    assert_matches_oracle(gpu_runs["asm_cut0"]["one_spectrum"], "one_spectrum")


def test_assembly_and_plain_c_loops_agree(gpu_runs):
    """the same input through the assembly loop and through the C++ step loop of k_jump_bin (HULK_JUMP_C=1): equal spectra, and
    the oracle's"""
    assert np.array_equal(gpu_runs["asm"]["one_spectrum"]["hist"], gpu_runs["plain_c"]["one_spectrum"]["hist"])
    assert_matches_oracle(gpu_runs["plain_c"]["one_spectrum"], "one_spectrum")
