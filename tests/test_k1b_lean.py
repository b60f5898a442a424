"""What k_jump_bin issues outside its step loop: compiles hulk_spectrum.hip to gfx950 assembly with the Makefile's flags, as
test_k1b_resources.py does, and counts in the text of the function (no GPU needed; skipped where hipcc is absent).

The step loop lives in inline-assembly blocks (the ones with a v_rcp_f64).  Its values are bound to the loop's fixed registers
by physical-register constraints, so a block is entered and left without copies: the only moves allowed in it are the two of
the odd exit (each block held 14 before).  Everything else the function issues on the vector ALU — round set-up, the stores,
the hand-over to the pool, the pool's compaction, and the C++ comparator loop (HULK_JUMP_C) — is counted statically: 141
before the lane masks stayed scalar and the hand-over's destination became a select on the mask, 103 since.  The bound is
that count plus two (a compiler's scheduling freedom), and may never be raised past 115."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hulk_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
VALU_OUTSIDE_MAX = 105          # 103 counted + 2
assert VALU_OUTSIDE_MAX <= 115


@pytest.fixture(scope="module")
def jump_bin_text(tmp_path_factory):
    """(inline-assembly blocks, compiler-generated lines) of k_jump_bin, each a list of stripped instruction lines"""
    if HIPCC is None:
        pytest.skip("hipcc not found")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    out = str(tmp_path_factory.mktemp("k1b_lean") / "hulk_spectrum.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-o", out,
                           os.path.join(CSRC, "hulk_spectrum.hip")], stderr=subprocess.DEVNULL)
    m = re.search(r"^(_Z\S*k_jump_bin\S*):[^\n]*\n(.*?)^\.Lfunc_end", open(out).read(), re.M | re.S)
    assert m, "k_jump_bin not found in the assembly"
    blocks, outside, cur = [], [], None
    for line in m.group(2).split("\n"):
        s = line.strip()
        if s.startswith(";;#ASMSTART"):
            cur = []
        elif s.startswith(";;#ASMEND"):
            blocks.append(cur)
            cur = None
        elif cur is not None:
            cur.append(s)
        elif s and not s.startswith((";", ".")) and not s.endswith(":"):
            outside.append(s)
    assert cur is None
    return blocks, outside


def step_blocks(blocks):
    return [b for b in blocks if any(l.startswith("v_rcp_f64") for l in b)]


def test_step_loop_blocks_hold_no_copies(jump_bin_text):
    blocks, _ = jump_bin_text
    loops = step_blocks(blocks)
    assert len(loops) == 3, len(loops)                       # main round, pool round, drain
    for b in loops:
        movs = [l for l in b if l.startswith("v_mov_b")]
        print(len(b), "lines,", movs)
        assert len(movs) <= 2, movs                           # the odd exit's fix-up and nothing else
        assert sum(l.startswith("v_rcp_f64") for l in b) == 2  # the two-step unroll
        # the lanes to work on arrive as a scalar mask (a lane mask the compiler took for divergent would arrive in a VGPR pair)
        assert re.match(r"s_and_saveexec_b64 s\[60:61\], s\[\d+:\d+\]$", b[0]), b[0]


def test_loop_constants_are_written_once(jump_bin_text):
    blocks, outside = jump_bin_text
    consts = [b for b in blocks if any(re.match(r"v_mov_b32 v47, 0x43300000$", l) for l in b)]
    assert len(consts) == 1 and not step_blocks(consts), blocks
    # ... and the compiler neither copies nor rebuilds them elsewhere
    assert not [l for l in outside if re.search(r"\bv(47|56|57|58)\b|v\[56:57\]", l)]


def test_valu_outside_the_step_loop(jump_bin_text):
    _, outside = jump_bin_text
    valu = [l for l in outside if l.startswith("v_")]
    by_op = {}
    for l in valu:
        by_op[l.split()[0]] = by_op.get(l.split()[0], 0) + 1
    print(len(valu), sorted(by_op.items(), key=lambda kv: -kv[1]))
    assert len(valu) <= VALU_OUTSIDE_MAX, (len(valu), by_op)
