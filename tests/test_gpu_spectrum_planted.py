"""The 4-bit spectrum (k_nibble_hist -> k_nibble_merge -> k_recount_flagged) and the exact path (k_range_hist -> k_merge_hist) on
the planted inputs of tests/spectrum_plant.py: counters at exactly 15 and at 16, in chosen parts, nibbles, words, ranges and ring
slots (tests/test_spectrum_plant_cpu.py shows that every input has the per-part counts it claims).

Every case is compared with the CPU oracle: histogram bin for bin, minimizer count, the histogram's sum, and — where the case has
several intervals — count-min counters and `mins` bit-exact and the weights to WEIGHT_RTOL after finish().  A wrong count is an
integer error; no tolerance applies to it.

Each case runs two ways.  On the profiling build, in a subprocess per environment setting (the knobs are read once per process),
where the hook HULK_DEBUG_NIBBLE also tells what the launch did: its geometry must be the one the Python mirror of the launch rule
predicts, and nib_over must be set exactly for the spectra in which a planted counter reaches 16 — agreement with the oracle alone
cannot tell "stayed on the merge path" from "was flagged and recounted".  And on the shipping library, in this process, against the
oracle only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import spectrum_plant as sp
from conftest import pack_reads
from oracle import pyorc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP_LIB = os.path.join(ROOT, "hulk_amd", "csrc", "libhulkhip_exp.so")
WEIGHT_RTOL = 1e-9
S = 16
RING_MAX = 17

_RUNNER = """
import json, sys, time
import numpy as np
sys.path.insert(0, {root!r})
import hulk_amd
from hulk_amd import _lib
assert _lib.load().hulk_build_info().endswith(b" experiments=1")
for name, k, interval, batch, lanes, cuts, finish in json.loads(sys.argv[2]):
    d = np.load(sys.argv[1] + "/" + name + ".npz")
    t0 = time.time()
    out = run_case(hulk_amd, d["bases"], d["offsets"], k, interval, batch, lanes, cuts, finish)
    np.savez(sys.argv[3] + "/" + name + ".npz", seconds=time.time() - t0, **out)
print("DONE", flush=True)
"""


def run_case(hulk_amd, bases, offsets, k, interval, batch, lanes, cuts, finish, hook=True):
    """one case through a GpuSketcher of whatever library this process loaded: the arrays that are compared with the oracle, and
    (hook) what HULK_DEBUG_NIBBLE reports after the last host call"""
    g = hulk_amd.GpuSketcher(k, 1, S, interval, batch=batch, work_lanes=lanes)
    try:
        for a, b in zip(cuts[:-1], cuts[1:]):
            g.add_reads(bases, offsets[a:b + 1])
        out = dict(nibble=g.debug_read(hulk_amd._lib.HULK_DEBUG_NIBBLE) if hook else np.zeros(0, np.uint32), hist=g.histogram(),
                   n_min=np.uint64(g.counters()["n_minimizers"]))
        if finish:
            try:
                g.finish()
            except hulk_amd.HulkError as e:                        # (reported per case: the other cases of the process still run)
                out["err"] = np.array(str(e))
                return out
            out["cms"] = g.cms()
            out["mins"], out["weights"] = g.sketch()
        return out
    finally:
        g.close()


def _cuts(c):
    return [0] + [int(x) for x in np.cumsum(c.calls)]


@pytest.fixture(scope="module")
def exp_runs(tmp_path_factory):
    """{leg: {case: arrays}}: every leg's cases through the profiling build, one subprocess per leg"""
    assert os.path.exists(EXP_LIB), "profiling build (libhulkhip_exp.so) not built"
    import inspect
    runner = "S = %d\n" % S + inspect.getsource(run_case) + _RUNNER.format(root=ROOT)
    knobs = {k for env, _ in sp.LEGS.values() for k in env}
    env0 = {k: v for k, v in os.environ.items() if k not in knobs}
    out = {}
    for leg, (env, names) in sp.LEGS.items():
        d_in, d_out = tmp_path_factory.mktemp("plant_in_" + leg), tmp_path_factory.mktemp("plant_out_" + leg)
        spec = []
        for n in names:
            c = sp.case(leg, n)
            bases, offsets = pack_reads(c.reads)
            np.savez(str(d_in / f"{n}.npz"), bases=bases, offsets=offsets)
            spec.append([n, c.k, c.interval, c.batch, c.work_lanes, _cuts(c), c.finish])
        r = subprocess.run([sys.executable, "-c", runner, str(d_in), json.dumps(spec), str(d_out)],
                           env=dict(env0, HULK_LIB="exp", **env), capture_output=True, text=True, timeout=240)
        assert r.returncode == 0 and "DONE" in r.stdout, f"{leg}: exit {r.returncode}: {r.stderr[-2000:]}"
        out[leg] = {n: dict(np.load(str(d_out / f"{n}.npz"))) for n in names}
        print(f"[spectrum_planted] leg {leg}: " + ", ".join(f"{n} {float(out[leg][n]['seconds']):.2f}s" for n in names))
    return out


_ORACLE, _SHARED = {}, {}


def oracle(leg, name):
    """the CPU oracle's result of a case (computed once).  A case without an interval never flushes before its histogram is read:
    those share one oracle per k, wiped in between (drawing its tables takes half a second)."""
    if (leg, name) not in _ORACLE:
        c = sp.case(leg, name)
        packed = pack_reads(c.reads)
        if not c.interval and not c.finish:
            if c.k not in _SHARED:
                _SHARED[c.k] = pyorc.Sketcher(c.k, 1, S, 0, 1.0, 0)
            o = _SHARED[c.k]
            o.wipe()
            before = o.counters()["n_minimizers"]
            o.add_reads(*packed)
            _ORACLE[(leg, name)] = dict(hist=o.histogram().astype(np.uint32), n_min=o.counters()["n_minimizers"] - before)
        else:
            o = pyorc.Sketcher(c.k, 1, S, 0, 1.0, c.interval)
            o.add_reads(*packed)
            res = dict(hist=o.histogram().astype(np.uint32), n_min=o.counters()["n_minimizers"])
            if c.finish:
                o.finish()
                res["cms"] = o.cms()
                res["mins"], res["weights"] = o.sketch()
            o.close()
            _ORACLE[(leg, name)] = res
    return _ORACLE[(leg, name)]


def assert_matches_oracle(got, leg, name):
    c, want = sp.case(leg, name), oracle(leg, name)
    assert int(got["n_min"]) == want["n_min"] == c.n
    diff = np.nonzero(got["hist"] != want["hist"])[0]
    assert not len(diff), f"{len(diff)} bins differ, first: " + ", ".join(f"bin {b}: {got['hist'][b]} != {want['hist'][b]}" for b in diff[:8])
    # the histogram that is read is the spectrum still open after the last call (all of the stream where there is no interval)
    open_reads = c.n - (c.n // c.interval) * c.interval if c.interval else c.n
    assert int(got["hist"].sum(dtype=np.uint64)) == open_reads, "spectrum increments lost or doubled"
    if c.finish:
        assert "err" not in got, f"finish() failed: {got['err']}"
        assert np.array_equal(got["cms"], want["cms"]), f"count-min counters differ in {int((got['cms'] != want['cms']).sum())} places"
        assert np.array_equal(got["mins"], want["mins"]), f"{int((got['mins'] != want['mins']).sum())} of {S} mins differ"
        assert np.allclose(got["weights"], want["weights"], rtol=WEIGHT_RTOL, atol=0)


@pytest.mark.parametrize("leg,name", sp.all_cases(), ids=[f"{leg}-{name}" for leg, name in sp.all_cases()])
def test_profiling_build_matches_oracle_geometry_and_flags(exp_runs, leg, name):
    """oracle equality, and through the hook: the launch had the geometry the mirror predicts (n_spectra, parts, ranges, log2 of the
    range, block size), and nib_over is set for exactly the spectra in which a planted counter reaches 16"""
    c, got = sp.case(leg, name), exp_runs[leg][name]
    nib = [int(x) for x in got["nibble"]]
    assert len(nib) == 5 + RING_MAX
    assert nib[:5] == c.launches[-1].geometry(), "the launch is not the one the mirror of the part rule predicts"
    n_spectra = nib[0]
    assert nib[5:5 + n_spectra] == c.flags(), "nib_over: flagged spectra are not the ones with a counter at 16"
    assert not any(nib[5 + n_spectra:])
    assert_matches_oracle(got, leg, name)


@pytest.mark.parametrize("name", list(sp.DEFAULT_CASES))
def test_shipping_library_matches_oracle(name):
    """the same cases through the library this process loads, oracle equality only (it has no hook)"""
    import hulk_amd
    c = sp.case("default", name)
    bases, offsets = pack_reads(c.reads)
    got = run_case(hulk_amd, bases, offsets, c.k, c.interval, c.batch, c.work_lanes, _cuts(c), c.finish, hook=False)
    assert_matches_oracle(got, "default", name)
