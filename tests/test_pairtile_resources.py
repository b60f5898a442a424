"""Registers, scratch and LDS of every kernel built on the pair tile (hulk_pairtile.h, hulk_bottomk_tile.h): compiles the six units to
gfx950 assembly with the Makefile's CXXFLAGS and reads the kernels' metadata (no GPU needed; skipped where hipcc is absent).

The tile keeps 16 accumulators, 4 unions and 16 counts a thread in registers across the slot loop: a spill or any scratch puts
loads and stores into that loop.  LDS decides how many workgroups share a CU (160 KiB): the tile's arrays are derived here from the
header's constants, and a kernel may add only the statics listed in STATICS.  Metadata fields only: no instruction is read."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hulk_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
UNITS = ("hulk_search", "hulk_cluster", "hulk_links", "hulk_dendrogram", "hulk_pairwise", "hulk_bottomk")
LDS_PER_CU = 160 * 1024
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size")

# the set type as it appears in a mangled kernel name -> (the set, workgroups per CU its tile admits)
SETS = {"7PairSetILi0EE": ("PairSet<0>", 3), "7PairSetILi1EE": ("PairSet<1>", 2), "10BottomkSet": ("BottomkSet", 4)}
# kernel -> (instances, bytes of its own statics, their source).  A 4-byte word behind arrays aligned to 8 or 16 costs 8.
STATICS = {
    "k_search_dist": (4, 0, "hulk_search.hip: none (PairSet<1> twice: the query as subject, the database sketch as subject)"),
    "k_cluster_link": (3, 8, "hulk_cluster.hip, cluster_link: __shared__ uint32_t wg_links"),
    "k_links_count": (3, 0, "hulk_links.hip: none"),
    "k_links_fill": (3, 0, "hulk_links.hip: none"),
    "k_dendro_offer": (3, 768, "hulk_dendrogram.hip, dendro_offer: __shared__ uint64_t x_d[PAIR_TQ]; uint32_t x_p[PAIR_TQ]"),
    "k_smash": (2, 0, "hulk_pairwise.hip: none (template <int METRIC>: the tile of PairSet<METRIC>)"),
    "k_bottomk_matrix": (1, 0, "hulk_bottomk.hip: none (takes a BottomkSet)"),
}


def tile_bytes():
    """what SET::tile declares, from the constants of the two headers"""
    pair = open(os.path.join(CSRC, "hulk_pairtile.h")).read()
    m = re.search(r"constexpr int PAIR_TS = (\d+), PAIR_TQ = (\d+), PAIR_CH = (\d+), PAIR_PAD = (\d+);", pair)
    ts, tq, ch, pad = (int(x) for x in m.groups())
    # double ma[2][CH][TS + PAD], mb[2][CH][TQ + PAD]; weighted: wa[2][CH][TS + PAD] (jaccard's wa[1][1][..] is never read and is dropped)
    assert re.search(r"double ma\[2\]\[PAIR_CH\]\[PAIR_TS \+ PAIR_PAD\], wa\[METRIC == 1 \? 2 : 1\]\[METRIC == 1 \? PAIR_CH : 1\]\[PAIR_TS \+ PAIR_PAD\];", pair)
    assert re.search(r"double mb\[2\]\[PAIR_CH\]\[PAIR_TQ \+ PAIR_PAD\];", pair)
    jaccard = 8 * 2 * ch * ((ts + pad) + (tq + pad))
    weighted = jaccard + 8 * 2 * ch * (ts + pad)
    bk = open(os.path.join(CSRC, "hulk_bottomk_tile.h")).read()
    w = int(re.search(r"constexpr int BK_W = (\d+), BK_PITCH = BK_W \+ 1, BK_LISTS = PAIR_TS \+ PAIR_TQ;", bk).group(1))
    lists = ts + tq
    # uint64 wv[LISTS][PITCH]; uint32 wm[LISTS][PITCH]; uint32 s_cur, s_len, s_n [LISTS]; uint64 s_piv[2]; uint32 s_more[2]
    for decl in ("uint64_t wv[BK_LISTS][BK_PITCH]", "uint32_t wm[BK_LISTS][BK_PITCH]", "uint32_t s_cur[BK_LISTS], s_len[BK_LISTS], s_n[BK_LISTS]",
                 "uint64_t s_piv[2]", "uint32_t s_more[2]"):
        assert decl in bk, decl
    bottomk = lists * (w + 1) * (8 + 4) + 3 * lists * 4 + 2 * 8 + 2 * 4
    return {"PairSet<0>": jaccard, "PairSet<1>": weighted, "BottomkSet": bottomk}


def test_tile_bytes_and_occupancy():
    t = tile_bytes()
    assert t == {"PairSet<0>": 51200, "PairSet<1>": 68608, "BottomkSet": 39192}
    for _, (name, wgs) in SETS.items():
        most = max(s for _, s, _ in STATICS.values())
        assert LDS_PER_CU // t[name] == wgs == LDS_PER_CU // (t[name] + most), (name, t[name], wgs)
    assert sum(n for n, _, _ in STATICS.values()) == 19


@pytest.fixture(scope="module")
def kernel_metadata(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    out = tmp_path_factory.mktemp("pairtile")

    def compile_unit(unit):
        path = str(out / (unit + ".s"))
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-o", path, os.path.join(CSRC, unit + ".hip")],
                              stderr=subprocess.DEVNULL)
        return open(path).read()
    meta = {}
    with ThreadPoolExecutor(max_workers=len(UNITS)) as pool:
        for text in pool.map(compile_unit, UNITS):
            for block in re.split(r"\n  - \.agpr_count", text)[1:]:
                name = re.search(r"\.name:\s+(\S+)", block)
                kernel = name and re.search(r"_GLOBAL__N_1\d+(k_[a-z_]+?)(I|E)", name.group(1))
                if kernel and kernel.group(1) in STATICS:
                    meta[name.group(1)] = (kernel.group(1), {f: int(v) for f, v in re.findall(r"\.(%s):\s+(\d+)" % "|".join(FIELDS), block)})
    return meta


def set_of(kernel, mangled):
    hits = [name for tag, (name, _) in SETS.items() if tag in mangled]
    if kernel == "k_smash":
        hits = ["PairSet<%s>" % re.search(r"k_smashILi(\d)E", mangled).group(1)]
    assert len(hits) == 1, mangled
    return hits[0]


def test_every_instance_is_built(kernel_metadata):
    seen = {}
    for mangled, (kernel, m) in kernel_metadata.items():
        seen.setdefault(kernel, []).append(set_of(kernel, mangled))
    for kernel, (instances, _, _) in STATICS.items():
        assert len(seen.get(kernel, [])) == instances, (kernel, seen.get(kernel))
        if instances >= 3:
            assert set(seen[kernel]) == {"PairSet<0>", "PairSet<1>", "BottomkSet"}, (kernel, seen[kernel])
    assert sorted(seen["k_smash"]) == ["PairSet<0>", "PairSet<1>"] and seen["k_bottomk_matrix"] == ["BottomkSet"]


def test_no_scratch_no_spill_and_the_tiles_lds(kernel_metadata):
    tiles = tile_bytes()
    assert len(kernel_metadata) == 19
    for mangled, (kernel, m) in sorted(kernel_metadata.items()):
        name = set_of(kernel, mangled)
        print(f"{kernel}<{name}>: {m}")
        assert set(m) == set(FIELDS), (mangled, m)
        assert m["max_flat_workgroup_size"] == 128, (mangled, m)
        assert m["private_segment_fixed_size"] == 0, (mangled, m)      # no scratch memory at all
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (mangled, m)
        assert m["vgpr_count"] <= 256, (mangled, m)                    # 128 threads: two waves, a quarter of a SIMD's 512 each and more
        assert m["group_segment_fixed_size"] == tiles[name] + STATICS[kernel][1], (mangled, m, STATICS[kernel][2])
        wgs = {n: w for n, w in SETS.values()}[name]
        assert LDS_PER_CU // m["group_segment_fixed_size"] == wgs, (mangled, m)
