"""Register budget of the k_minimizer_fast instances that are built for five workgroups per CU: compiles hulk_minimizer.hip to
gfx950 assembly and reads the kernels' metadata (no GPU needed; skipped where hipcc is absent).

A 256-thread workgroup is one wave per SIMD, so five workgroups per CU need <= 96 VGPRs (512 / 5, in granules of 8); six
would need <= 80.  `.sgpr_count` <= 96 keeps the scalar side out of the way (up to 96 admit seven workgroups).  Nothing may
be spilled: a spill of a loop-invariant value is reloaded inside the main loop.  The LDS side of the same occupancy is
tied down by static_asserts next to minimizer_fast_lds()."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hulk_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

VGPR_BUDGET = {5: 96, 6: 80}
# <WM, FM, DBG, WEQ, KC, PAIR> -> workgroups per CU the instance declares (fast_blocks_per_cu in hulk_minimizer.hip)
INSTANCES = {
    "k=21 (headline)": ("ILi9ELb1ELb0ELb1ELi21ELb0EE", 5),
    "k=21 PAIR": ("ILi9ELb1ELb0ELb1ELi21ELb1EE", 5),
    "k=31": ("ILi9ELb0ELb0ELb1ELi31ELb0EE", 5),
    "k=31 PAIR": ("ILi9ELb0ELb0ELb1ELi31ELb1EE", 5),
}


@pytest.fixture(scope="module")
def kernel_metadata(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    out = str(tmp_path_factory.mktemp("k1a") / "hulk_minimizer.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-o", out,
                           os.path.join(CSRC, "hulk_minimizer.hip")], stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = {}
    for block in re.split(r"\n  - \.agpr_count", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name and "k_minimizer_fast" in name.group(1):
            meta[name.group(1)] = {f: int(v) for f, v in re.findall(r"\.(vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|"
                                                                      r"private_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)", block)}
    assert meta, "no k_minimizer_fast kernel in the assembly's metadata"
    return meta


@pytest.mark.parametrize("which", sorted(INSTANCES))
def test_register_budget_of_the_declared_occupancy(kernel_metadata, which):
    tag, blocks = INSTANCES[which]
    hits = [m for n, m in kernel_metadata.items() if "k_minimizer_fast" + tag in n]
    assert len(hits) == 1, (which, len(hits))
    m = hits[0]
    print(which, m)
    assert m["max_flat_workgroup_size"] == 256
    assert m["vgpr_count"] <= VGPR_BUDGET[blocks], (which, m)
    assert m["sgpr_count"] <= 96, (which, m)
    assert m["vgpr_spill_count"] == 0, (which, m)
    assert m["sgpr_spill_count"] == 0, (which, m)
    assert m["private_segment_fixed_size"] == 0, (which, m)          # no scratch memory at all


def test_declared_blocks_match_the_source():
    """The table above against fast_blocks_per_cu(): 5 for WM = 9, WEQ, k fixed at 21 or 31, not the debug instance."""
    src = open(os.path.join(CSRC, "hulk_minimizer.hip")).read()
    assert re.search(r"return \(WM == 9 && !DBG && WEQ && \(KC == 21 \|\| KC == 31\)\) \? 5 : 4;", src)
    assert all(b == 5 for _, b in INSTANCES.values())
