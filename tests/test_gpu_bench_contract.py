"""bench.py contract on the GPU box: ONE JSON line on stdout with the required keys; every secondary leg fault-isolated; the
sharded-step path through RCCL at world size 1; and `bench.py --gpus 2` / `--gpus 8` END TO END — self-spawn, the pre-warm
agreement, the other modes, value_c4 with ranks that hold none of the ragged last step, and the JSON relay — with all ranks
on this box's one GPU over the library's host transport (HULK_BENCH_TRANSPORT=gloo)."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
            "scaling", "vs_baseline", "dtype", "data", "config", "roofline")


def _keep(name, p):
    """stdout / stderr of a bench.py run of this suite, kept under gpurun_out/ (scratch): an intermittent failure of a multi-rank
    run can then be read afterwards (one was seen once in ~60 runs of the two-rank test, on a fresh box, without its text)."""
    try:
        d = os.path.join(ROOT, "gpurun_out")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f"contract_{name}.txt"), "w") as fh:
            fh.write(f"returncode {p.returncode}\n---- stdout\n{p.stdout[-20000:]}\n---- stderr\n{p.stderr[-20000:]}\n")
    except OSError:
        pass


def _run(extra, env_extra=None, timeout=900, full=True):
    """one bench.py run at N = 1; full: with --full (the secondary legs), else the plain run the driver times"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", HULK_BENCH_PREWARM_S="0",   # (no need to warm the GPU for a contract test)
               HULK_BENCH_LONG_STEPS="6")
    env.update(env_extra or {})
    if "--c3" in extra:                                      # (the C3 / C5 legs only where a test looks at them)
        extra = [x for x in extra if x != "--c3"]
    else:
        extra = extra + ["--no-c3", "--no-c5", "--no-long-reads"]
    if full:
        extra = ["--full"] + extra
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2"] + extra,   # (2: both work lanes have run once before the clock starts)
                       capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_json_contract_and_collective_path():
    a = _run(["--no-cpu-baseline", "--c3"])
    for k in REQUIRED:
        assert k in a, k
    assert not [k for k in a if k.endswith("_error")], [k for k in a if k.endswith("_error")]
    # the timed pass carries no event brackets; the kernel durations come from the one-stream `kernels` leg
    assert "no HIP-event brackets" in a["timed_pass_note"] and "HULK_FLAG_NO_OVERLAP" in a["roofline"]["durations_from"]
    assert a["ms_per_step_kernels_alone"] > 0.8 * a["ms_per_step"]
    assert a["steps_long"] == 6 and 0.5 * a["ms_per_step"] < a["ms_per_step_long"] < 2.0 * a["ms_per_step"]
    # BASELINE configs[2] and [4] are in the driver's line
    c3 = a["c3"]
    assert "k=31" in c3["workload"] and c3["reads"] >= 8_000_000 and 1e8 < c3["value"] < a["value"]
    assert c3["negative_weights"] == 1024 and c3["kernels_alone"]["k_cmsd_freq_us"] > 0 and c3["kernels_alone"]["k_minimizer_fast_us"] > 0
    c5 = a["c5"]
    for metric in ("weightedjaccard", "jaccard"):
        assert c5[metric]["ms_kernel"] < c5[metric]["ms_end_to_end"] and 0.0 < c5[metric]["valu_frac"] < 1.0
    assert c5["pairs"] == 1024 * 1024
    # ... and the command as the reference runs it: 1024 sketch files in, MD5-verified, the same matrix out
    assert c5["directory"]["files"] == 1024 and c5["directory"]["same_matrix_as_arrays"] and c5["directory"]["seconds_load_and_md5"] > 0
    assert a["n_gpus"] == 1 and a["steps"] == 3 and a["warmup"] == 2 and a["vs_baseline"] is None
    assert a["unit"] == "reads/s" and a["higher_is_better"] is True and a["scaling"] == "weak"
    assert "workload" in a["config"] and "model" not in a["config"]
    r = a["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    # algorithmic bytes = SURVEY.md §8(d)'s per-read figure (L + 8) x the reads of one launch; nothing else priced in
    assert r["alg_bytes_per_launch"] == a["config"]["reads_per_rank_step"] * (150 + 8) and r["traffic"] == r["traffic_from_profile"]     # (PMC passes of the same command: profiles/r05_pmc.json)
    assert abs(r["achieved"] - r["alg_bytes_per_launch"] / (r["avg_launch_us"] * 1e-6) / 1e9) < 1e-6 * r["achieved"]
    # the line names the longest single kernel from the durations it measured itself
    assert r["longest_kernel"] == ("k_minimizer_fast" if r["avg_launch_us"] >= a["k_jump_bin"]["avg_launch_us"] else "k_jump_bin")
    assert a["k_jump_left"]["avg_launch_us"] < a["k_jump_bin"]["avg_launch_us"]
    assert a["value"] > 1e7 and abs(a["ms_per_step"] * a["value"] / 1e3 - a["config"]["reads_per_step"]) < 1.0
    assert a["rccl_ranks"] == 0 and a["collective"] is None
    # C2 exactly as BASELINE states it: 10 M reads on a fresh context; below the steady-state rate, above 1e8
    assert a["cold_reads"] == 10_000_000 and 1e8 < a["value_cold"] < 1.2 * a["value"]
    # ... and the same run with the GPU's clocks ramped between hulk_create and the first read: idle clocks separated from code
    assert 1e8 < a["value_cold_ramped"] < 1.2 * a["value"] and len(a["cold_ramped_seconds_all_runs"]) == 2
    # sequences beyond the short-read kernels: 5 kb reads and 500 kb contigs (sketch.go:102-135), a rate, a kernel table, a roofline
    lr = a["long_reads"]
    for shape, n, L in (("reads_5kb", 200_000, 5_000), ("contigs_500kb", 2_000, 500_000)):
        x = lr[shape]
        assert x["sequences"] == n and x["length"] == L and x["bases_per_s"] > 1e9 and x["reads_per_s"] * L == pytest.approx(x["bases_per_s"])
        assert x["kernels_alone"]["us"]["k_long_tile"] > 0
        r_ = x["roofline_k_long_tile"]
        assert r_["bound"] == "hbm" and 0 < r_["frac"] < 1 and abs(r_["frac"] - r_["achieved"] / r_["peak"]) < 1e-12
        assert 150 < x["minimizers_per_kb"] < 250                # ~2 / (w + 1) distinct minimizers per position of a random sequence
    fa = lr["fasta_file"]                                          # the reference's --fasta mode from a file: same sketch as the same contigs in HBM
    assert fa["contigs"] == 200 and fa["bases_per_s"] > 1e8 and fa["same_sketch_as_device_buffers"] is True
    assert a["value_unpruned"] is not None and a["value_unpruned"] <= 1.2 * a["value"]
    # end to end from a FASTQ file, plain and .gz: host-bound, far below the kernel-path rate, same sketch both ways
    e2e = a["e2e"]
    # (one member inflated by several threads and bgzip'd members side by side: both well above one inflate thread's ~5e6, neither
    # ordered against the other nor — on a noisy host — strictly against the plain file)
    for c in ("plain", "gz", "bgzf"):
        assert 1e5 < e2e[c]["value"] < a["value"] and e2e[c]["sketch_md5"] == e2e["plain"]["sketch_md5"]
        assert len(e2e[c]["seconds_all_runs"]) == 4 and min(e2e[c]["seconds_all_runs"]) == e2e[c]["seconds"]
        assert e2e[c]["parse_only_reads_per_s"] > 1e5
    assert e2e["gz"]["value"] < 1.5 * e2e["plain"]["value"] and e2e["bgzf"]["value"] < 1.5 * e2e["plain"]["value"]
    # 8 M reads with the line machine on the device and on the host's parser threads: same sketch
    assert e2e["plain_8m"]["reads"] == 8_000_000 and e2e["plain_8m"]["sketch_md5"] == e2e["plain_8m_host_parser"]["sketch_md5"]
    assert e2e["plain_8m"]["value"] > 1e6 and e2e["plain_8m_host_parser"]["value"] > 1e6
    # the sharded step at world size 1: RCCL communicator, exchange inside the library, same sketch
    b = _run(["--no-cpu-baseline", "--no-cold", "--force-collective"], {"HULK_BENCH_C4_READS_PER_RANK": "5000000"})
    assert b["sketch_md5"] == a["sketch_md5"]
    assert b["rccl_ranks"] == 1                         # dist.get_world_size() on the nccl (= RCCL) backend
    cs = b["collective"]["timed_pass"]
    assert "RCCL" in b["collective"]["transport"] and cs["steps_full"] >= 1 and cs["steps_delta"] >= 1
    assert [o["mode"] for o in b["other_scaling"]] == ["sliced-strong", "sliced-weak"]
    for o in b["other_scaling"]:                        # at one rank every mode is the same work and the same sketch
        assert o["reads_per_rank_step"] == b["config"]["reads_per_rank_step"] and 0.5 * b["value"] < o["value"] < 2.0 * b["value"]
        assert o["sketch_md5"] == a["sketch_md5"]
    assert "other_scaling" not in a and "value_c4" not in a
    assert b["c4_reads"] == 5_000_000 and b["c4_exchange"]["steps_delta"] >= 1 and 1e8 < b["value_c4"] < 1.2 * b["value"]
    # SURVEY.md 8(e)'s slice split as the headline: same stream, same interval, same sketch
    f = _run(["--no-cpu-baseline", "--single-pass", "--mode", "sliced-strong", "--force-collective"])
    assert f["sketch_md5"] == a["sketch_md5"] and "slice" in f["config"]["split"] and "whole" in a["config"]["split"]
    assert f["scaling"] == "strong" and "all-reduce" in f["collective"]["per_step"]
    # the real unpruned switch: the timed pass itself reads the whole table for every interval, same sketch
    c = _run(["--no-cpu-baseline", "--no-cold", "--no-e2e", "--no-prune"])
    assert c["sketch_md5"] == a["sketch_md5"]
    sc, sa = c["roofline_cws_scan"], a["roofline_cws_scan"]
    assert sc["tiles_read_per_launch"] == sc["tiles_covered_per_launch"] > 0
    assert sa["tiles_read_per_launch"] < sc["tiles_read_per_launch"]
    assert sc["avg_launch_us"] > sa["avg_launch_us"]
    # variant: 1 % of the reads carry an N (they leave the fast minimizer kernel): measured -2 %, must stay within 15 % here
    e = _run(["--no-cpu-baseline", "--no-cold", "--no-e2e", "--single-pass", "--n-frac", "0.01"])
    assert e["sketch_md5"] != a["sketch_md5"] and e["value"] > 0.85 * a["value"]
    assert "VARIANT" in e["config"]["workload"]
    # one rank's share of an 8-rank step without peers (projection aid): labelled, never a headline
    g = _run(["--no-cpu-baseline", "--single-pass", "--loopback", "8"])
    assert "LOOPBACK" in g["config"]["workload"] and g["config"]["reads_per_step"] == 8 * g["config"]["reads_per_rank_step"]


def test_bench_line_survives_any_secondary_leg():
    """Fault isolation: every secondary leg may raise (HULK_BENCH_FAIL names the legs that do) and the ONE line still comes
    out with the headline in it, `<leg>_error` for each of them, and exit status 0."""
    ok = _run(["--no-cpu-baseline", "--single-pass", "--no-cold", "--no-e2e"])
    legs = "kernels,unpruned,long,cold,c3,long_reads,c5,e2e,cpu_baseline"
    a = _run(["--c3"], {"HULK_BENCH_FAIL": legs})
    for leg in legs.split(","):
        assert "HULK_BENCH_FAIL" in a[leg + "_error"], leg
    assert a["value"] > 1e7 and a["sketch_md5"] == ok["sketch_md5"] and a["roofline"] is None
    for gone in ("value_unpruned", "ms_per_step_long", "value_cold", "c3", "long_reads", "c5", "e2e", "cpu_baseline"):
        assert gone not in a, gone
    # at N > 1 (here: world 1 through the collective path) the modes and C4 each on their own; a failed collective leg
    # makes the ranks skip the collective legs behind it (they may no longer be in step), never the line
    b = _run(["--no-cpu-baseline", "--no-cold", "--no-e2e", "--force-collective"],
             {"HULK_BENCH_FAIL": "other_scaling_sliced-weak", "HULK_BENCH_C4_READS_PER_RANK": "3300000"})
    assert b["sketch_md5"] == ok["sketch_md5"] and "HULK_BENCH_FAIL" in b["other_scaling_sliced-weak_error"]
    assert [o["mode"] for o in b["other_scaling"]] == ["sliced-strong"] and "skipped" in b["c4_error"] and "value_c4" not in b
    # a leg that never returns: the watchdog prints the line and ends the process with status 0
    c = _run(["--no-cpu-baseline", "--single-pass", "--no-cold", "--no-e2e"], {"HULK_BENCH_HANG": "kernels", "HULK_BENCH_LEG_TIMEOUT_S": "8"})
    assert c["sketch_md5"] == ok["sketch_md5"] and "timeout" in c["kernels_error"] and c["roofline"] is None


def test_plain_run_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """Without --full a run is setup, the discarded passes and the headline: none of the secondary legs' keys in the line.
    --dump-outputs writes the sketch the timed pass ended with and the count-min counters as float64 .npy files — the
    sketch the line's sketch_md5 names — and a second run with the same arguments writes the same arrays."""
    import numpy as np
    a = _run(["--dump-outputs", str(tmp_path / "a")], full=False)
    for k in REQUIRED:
        assert k in a, k
    assert a["steps"] == 3 and a["warmup"] == 2 and a["roofline"] is None
    assert abs(a["ms_per_step"] * a["value"] / 1e3 - a["config"]["reads_per_step"]) < 1.0
    assert not [k for k in a if k.endswith("_error")], [k for k in a if k.endswith("_error")]
    for gone in ("ms_per_step_kernels_alone", "value_unpruned", "ms_per_step_long", "value_cold", "c3", "long_reads", "c5", "e2e",
                 "cpu_baseline", "other_scaling", "value_c4"):
        assert gone not in a, gone
    b = _run(["--dump-outputs", str(tmp_path / "b")], full=False)
    assert b["sketch_md5"] == a["sketch_md5"]
    shapes = {"sketch_mins": (512,), "sketch_weights": (512,), "countmin": (7, 2000)}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in shapes)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    for name, shape in shapes.items():
        x, y = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert x.dtype == np.float64 and x.shape == shape and np.array_equal(x, y), name
    mins = np.load(tmp_path / "a" / "sketch_mins.npy")
    assert hashlib.md5(mins.astype("<u8").tobytes()).hexdigest() == a["sketch_md5"]
    assert np.load(tmp_path / "a" / "countmin.npy").sum() > 0


def test_bench_says_so_when_rccl_cannot_be_bound():
    """hulk_comm_init failing (here: HULK_RCCL_LIB names a file that is not there) must not leave a scaling run without a
    line: every rank learns of it, the run goes over the library's host transport on a gloo group and the line says so."""
    a = _run(["--no-cpu-baseline", "--single-pass", "--no-cold", "--no-e2e", "--no-c4", "--force-collective"], {"HULK_RCCL_LIB": "/nonexistent/librccl.so.1"})
    t = a["collective"]["transport"]
    assert "host transport over gloo" in t and "RCCL unavailable" in t and "librccl" in t
    cs = a["collective"]["timed_pass"]
    assert cs["steps_full"] >= 1 and cs["steps_delta"] >= 1
    b = _run(["--no-cpu-baseline", "--single-pass", "--no-cold", "--no-e2e"])
    assert a["sketch_md5"] == b["sketch_md5"]


_one_rank = {}


def _one_rank_run(key, extra):
    """single-rank comparison runs, shared between the transports of the world-two test"""
    if key not in _one_rank:
        _one_rank[key] = _run(extra)
    return _one_rank[key]


@pytest.mark.parametrize("transport", ["gloo", "fakerccl"])
def test_bench_world_two_end_to_end_on_one_gpu(transport):
    """`python bench.py --gpus 2` the way the driver invokes it (no launcher), both ranks on GPU 0 — over the library's host
    transport (gloo) and over its RCCL branch (fakerccl: hulk_comm_init / ncclAllGather / ncclAllReduce bound to the test double
    tests/cpp/libfakerccl.so, the code path real RCCL ranks take): everything bench.py does at N > 1 runs — self_spawn, the
    pre-warm agreement, all three modes, value_c4 with its ragged last step, the JSON relay — and the sharded sketch is the
    single-GPU sketch of the same 2 x longer stream."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(HULK_BENCH_TRANSPORT=transport, HULK_BENCH_PREWARM_S="0.3", HULK_BENCH_C4_READS_PER_RANK="4100000")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=1200, env=env, cwd=ROOT)
    _keep("world_two_" + transport, p)                        # (what the two ranks printed: gpurun_out/contract_world_two_<transport>.txt)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    for k in REQUIRED:
        assert k in out, k
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["config"]["mode"] == "sharded"
    assert out["config"]["reads_per_step"] == 2 * out["config"]["reads_per_rank_step"] == 3_200_000
    assert abs(out["ms_per_step"] * out["value"] / 1e3 - out["config"]["reads_per_step"]) < 1.0
    cs = out["collective"]["timed_pass"]
    assert cs["steps_full"] >= 1 and cs["steps_delta"] >= 1 and cs["bytes_received"] > 0
    assert cs["headers_refetched"] == 0 and cs["void_blocks"] == 0, cs
    assert ("test double" in out["collective"]["transport"]) == (transport == "fakerccl"), out["collective"]["transport"]
    assert not [k for k in out if k.endswith("_error")], {k: out[k] for k in out if k.endswith("_error")}
    assert [o["mode"] for o in out["other_scaling"]] == ["sliced-strong", "sliced-weak"]
    # value_c4: 2 x 4.1 M reads = 82 intervals = 2 whole steps of 32 + a ragged one of 18 (rank 0: 16, rank 1: 2)
    assert out["c4_reads"] == 8_200_000 and out["c4_steps"] == 3 and out["value_c4"] > 1e6      # (a rate over a host path on one GPU: only that it ran)
    # the same global stream on ONE rank (4 steps of 32 intervals = 8 plain steps of 16): the same sketch
    one = _one_rank_run("six", ["--no-cpu-baseline", "--no-cold", "--no-e2e", "--single-pass", "--steps", "6", "--warmup", "2"])
    assert one["config"]["total_reads"] == 6 * 1_600_000
    assert out["sketch_md5"] == one["sketch_md5"]
    strong = [o for o in out["other_scaling"] if o["mode"] == "sliced-strong"][0]
    half = _one_rank_run("three", ["--no-cpu-baseline", "--no-cold", "--no-e2e", "--single-pass", "--steps", "3", "--warmup", "1"])
    assert strong["sketch_md5"] == half["sketch_md5"]


def test_bench_world_eight_end_to_end_on_one_gpu():
    """`python bench.py --gpus 8` — the driver's N = 8 invocation — with the eight ranks on GPU 0 over the host transport.
    C4 is laid out so that its ragged last step leaves ranks 2..7 WITHOUT any interval (8 x 1.85 M reads = 148 intervals = one
    whole step of 128 + one of 20: rank 0 holds 16, rank 1 four), the case that only exists from world 3 up; the sharded
    sketch must be the single-rank sketch of the same 8 x longer stream, C4's the single-rank sketch of its 14.8 M reads."""
    import hashlib
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(HULK_BENCH_TRANSPORT="gloo", HULK_BENCH_PREWARM_S="0", HULK_BENCH_C4_READS_PER_RANK="1850000", HULK_BENCH_LONG_STEPS="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1",
                        "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=1800, env=env, cwd=ROOT)
    _keep("world_eight", p)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    for k in REQUIRED:
        assert k in out, k
    assert not [k for k in out if k.endswith("_error")], {k: out[k] for k in out if k.endswith("_error")}
    assert out["n_gpus"] == 8 and out["scaling"] == "weak" and out["config"]["mode"] == "sharded"
    assert out["config"]["reads_per_step"] == 8 * out["config"]["reads_per_rank_step"] == 12_800_000
    assert abs(out["ms_per_step"] * out["value"] / 1e3 - out["config"]["reads_per_step"]) < 1.0
    cs = out["collective"]["timed_pass"]
    assert cs["steps_full"] + cs["steps_delta"] == 3 and cs["steps_full"] >= 1 and cs["steps_delta"] >= 1 and cs["bytes_received"] > 0
    assert [o["mode"] for o in out["other_scaling"]] == ["sliced-strong", "sliced-weak"]
    assert out["c4_reads"] == 14_800_000 and out["c4_steps"] == 2
    ce = out["c4_exchange"]
    assert ce["steps_full"] + ce["steps_delta"] == 2 and ce["steps_full"] >= 1
    # the same global stream on ONE rank: 3 steps of 128 intervals = 24 plain steps of 16
    one = _run(["--no-cpu-baseline", "--no-cold", "--no-e2e", "--single-pass", "--steps", "16", "--warmup", "8"])
    assert one["config"]["total_reads"] == 16 * 1_600_000
    assert out["sketch_md5"] == one["sketch_md5"]
    # C4's stream on one rank through the plain interval rule
    import torch
    import hulk_amd
    from hulk_amd import synth
    g = hulk_amd.GpuSketcher(21, 9, 512, interval=100_000)
    for first in range(0, 14_800_000, 1_600_000):
        n = min(1_600_000, 14_800_000 - first)
        b, off = synth.reads_torch(first, n, 150)
        torch.cuda.synchronize()
        g.add_reads_device(b.data_ptr(), off.data_ptr(), n, 150, b.numel())
        g.synchronize()
    g.finish()
    m, _ = g.sketch()
    g.close()
    assert out["c4_sketch_md5"] == hashlib.md5(m.astype("<u8").tobytes()).hexdigest()


def test_bench_gpus_2_spawns_or_refuses():
    """Invoked the way the driver invokes it (`python bench.py --gpus 2`, no launcher): on a one-GPU box it must refuse
    with a non-zero exit — never print an n_gpus: 1 line; with two GPUs it spawns two RCCL ranks."""
    import torch
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    if torch.cuda.device_count() < 2:
        assert p.returncode != 0 and "GPU(s) visible" in p.stderr and "{" not in p.stdout
    else:
        assert p.returncode == 0, p.stderr[-2000:]
        out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
        assert out["n_gpus"] == 2 and out["rccl_ranks"] == 2 and out["scaling"] == "weak"
