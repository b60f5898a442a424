"""k_jump_bin's step loop takes the lanes it works on as a scalar mask and hands back the live ones as one: the lanes outside
that mask at entry — the tail of a round with fewer than 64 values, the positions of a pool with fewer than 64 chains — must
come out as not live, keep their state and store nothing.

The cases are a few reads only, so that EVERY round is such a round: 1, 2, 3 and 5 random 150-base reads (w = 9) leave last rounds of
28, 51, 19 and 1 values at k = 21 and of 25, 51, 7 and 59 at k = 31, where the minimizer fills all 64 bits of the chain's key.
Settings of the profiling build: the default; single-chain hand-overs (cut 1 / pcut 1); nearly every chain through the pool
(cut 63 / pcut 1: a round of fewer than 64 values ends after its first step and the whole of it is pooled and drained); no pool
(cut 0); the C++ comparator loop.  One subprocess per setting, HULK_POISON=0xff: a chain that is never stored leaves a key of
0xffffffff, which no spectrum counts, so it shows as a lost increment.  The harness is test_gpu_jump_pool.py's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import pack_reads
from oracle import pyorc
import test_gpu_jump_pool as harness

pytestmark = pytest.mark.gpu

CASES = {f"k{k}_reads_{n}": (k, 0, 0, harness.random_reads(100 * k + n, n), [0, n]) for k in (21, 31) for n in (1, 2, 3, 5)}
SETTINGS = {
    "default": {},
    "cut1_pcut1": {"HULK_JUMP_CUT": "1", "HULK_JUMP_PCUT": "1"},
    "cut63_pcut1": {"HULK_JUMP_CUT": "63", "HULK_JUMP_PCUT": "1"},
    "cut0": {"HULK_JUMP_CUT": "0"},
    "plain_c": {"HULK_JUMP_C": "1"},
}


@pytest.fixture(scope="module")
def gpu_runs(tmp_path_factory):
    """{setting: {case: arrays}}: all cases through the profiling build, one subprocess per setting"""
    assert os.path.exists(harness.EXP_LIB), "profiling build (libhulkhip_exp.so) not built"
    d_in = tmp_path_factory.mktemp("lean_in")
    for name, (k, interval, batch, seqs, cuts) in CASES.items():
        bases, offsets = pack_reads(seqs)
        np.savez(str(d_in / f"{name}.npz"), bases=bases, offsets=offsets)
    env0 = {k: v for k, v in os.environ.items() if k not in harness.SWITCHES}
    spec = json.dumps([[n, c[0], c[1], c[2], c[4]] for n, c in CASES.items()])
    out = {}
    for setting, env in SETTINGS.items():
        d_out = tmp_path_factory.mktemp("lean_" + setting)
        r = subprocess.run([sys.executable, "-c", harness._RUNNER.format(root=harness.ROOT, S=harness.S), str(d_in), spec, str(d_out)],
                           env=dict(env0, HULK_LIB="exp", HULK_POISON="0xff", **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "DONE" in r.stdout, f"{setting}: {r.stderr[-2000:]}"
        out[setting] = {n: dict(np.load(str(d_out / f"{n}.npz"))) for n in CASES}
    return out


@pytest.fixture(scope="module")
def oracle_runs():
    """{case: (spectrum, n_minimizers)} of the CPU oracle, computed once"""
    out = {}
    for name, (k, interval, batch, seqs, cuts) in CASES.items():
        o = pyorc.Sketcher(k, 9, harness.S, 0, 1.0, interval)
        o.add_reads(*pack_reads(seqs))
        out[name] = (o.histogram().astype(np.uint32), o.counters()["n_minimizers"])
        o.close()
    return out


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_short_rounds_match_the_oracle(gpu_runs, oracle_runs, setting, name):
    got, (want_hist, want_n) = gpu_runs[setting][name], oracle_runs[name]
    n_last = want_n % 64
    print(name, setting, "n_minimizers", want_n, "last round", n_last)
    assert want_n < 64 * len(CASES[name][3]) and n_last != 0           # under 64 values per read: the last round is short
    assert int(got["n_min"]) == want_n
    assert np.array_equal(got["hist"], want_hist), f"{int((got['hist'] != want_hist).sum())} bins differ"
    assert int(got["hist"].sum(dtype=np.uint64)) == want_n, "spectrum increments lost"


@pytest.mark.parametrize("name", list(CASES))
def test_spectrum_is_identical_across_settings(gpu_runs, name):
    want = gpu_runs["default"][name]["hist"]
    for setting in SETTINGS:
        got = gpu_runs[setting][name]["hist"]
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), setting
