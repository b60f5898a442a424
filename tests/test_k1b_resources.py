"""Resources of k_jump_bin: compiles hulk_spectrum.hip to gfx950 assembly with the Makefile's flags and reads the kernels'
metadata (no GPU needed; skipped where hipcc is absent).

k_jump_bin runs beside the other work lane's k_minimizer_fast, which leaves a CU 3,840 B of LDS: the pool of slow chains is
therefore held in registers (moved with ds_permute_b32, which allocates nothing) and the kernel may declare no LDS at all.
<= 64 VGPRs keep its 8 waves per SIMD (65 would cost one); nothing may be spilled into the step loop's way."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hulk_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
FIELDS = ("agpr_count|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
          "group_segment_fixed_size|max_flat_workgroup_size")


@pytest.fixture(scope="module")
def kernel_metadata(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    out = str(tmp_path_factory.mktemp("k1b") / "hulk_spectrum.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-o", out,
                           os.path.join(CSRC, "hulk_spectrum.hip")], stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = {}
    for block in re.split(r"\n  - (?=\.agpr_count)", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            meta[name.group(1)] = {f: int(v) for f, v in re.findall(r"\.(" + FIELDS + r"):\s+(\d+)", block)}
    assert meta, "no kernel in the assembly's metadata"
    return meta


def test_k_jump_bin_keeps_eight_waves_per_simd_and_no_lds(kernel_metadata):
    hits = [m for n, m in kernel_metadata.items() if "k_jump_bin" in n]
    assert len(hits) == 1, sorted(kernel_metadata)
    m = hits[0]
    print(m)
    assert m["vgpr_count"] <= 64, m
    assert m["agpr_count"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["private_segment_fixed_size"] == 0, m          # no scratch memory at all
    assert m["group_segment_fixed_size"] == 0, m            # no static LDS (the launch passes no dynamic LDS either)
    assert m["max_flat_workgroup_size"] == 256, m


def test_k_jump_left_is_gone(kernel_metadata):
    assert not [n for n in kernel_metadata if "k_jump_left" in n]
    assert len(kernel_metadata) > 5                           # (the other kernels of the file are there: the parse works)
