"""The paired step of k_jump_bin (hulk_spectrum.hip): two jump steps share one v_rcp_f64, and a two-instruction guard sends the
lanes whose approximate product could sit on the wrong side of an integer through one exact step.  The profiling build's
hulk_debug_jump runs chosen 64-bit values through the kernel alone and returns the bins and the number of guarded lane-steps.

The reference is the reference's formula in pure Python (Python floats are IEEE doubles):
    j = int(float(b + 1) * (float(1 << 31) / float(r))),  r = (key >> 33) + 1,  key <- key * a + 1 before every step.
Step i (from 0) reads the key after i + 1 advances.  Constructed keys are made backwards: the key of step i is chosen (its upper
31 bits are r_i - 1), key_0 follows by inverting the LCG i + 1 times, and the chain from key_0 decides b_i; candidates are drawn
with numpy until enough of them have the property wanted, and every case then asserts that property in plain Python.

Q = n exactly (case "exit_eq"): n = k^4 is odd at k = 21 and 31, so r_i * n = (b_i + 1) * 2^31 needs r_i = 2^31 and b_i = n - 1, a
chain that has climbed to the last bin and then draws the one largest divisor.  Such keys are rare — search_exit_eq below finds
them at a rate of about 2^-22 per candidate at k = 21, steps 7 and 8 (none among 2^26 candidates each at steps 1 to 4), and
three among 2^27 candidates each at k = 31, steps 7 and 8 — so the ones it found once are listed (EXIT_EQ) instead of being
searched for in every run, with one of step 4 at k = 21; they assert their precondition like every other case.
The bin of such a key is n - 1 whichever way the product is rounded (a lane that stays does so with t = n - 1 and leaves at the
next step), so what the case checks is the guard counter: every one of them must take the exact step.

Every setting of the profiling build runs all arrays in one child process (the switches are read once per process), as in
test_gpu_jump_pool.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP_LIB = os.path.join(ROOT, "hulk_amd", "csrc", "libhulkhip_exp.so")
SWITCHES = ("HULK_JUMP_CUT", "HULK_JUMP_PCUT", "HULK_JUMP_REGIONS", "HULK_JUMP_C", "HULK_JUMP_NO_GUARD", "HULK_JUMP_LDS")
A = 2862933555777941757
A_INV = pow(A, -1, 1 << 64)
M64 = (1 << 64) - 1
KS = (21, 31)
STEPS = (1, 2, 3, 4, 7, 8)               # both halves of a trip
REGION_LENS = (1, 63, 64, 65, 449)
PER_STEP_EXACT = 200                    # half with r_i a power of two, half with r_i = o * 2^j, o odd > 1
PER_STEP_EXIT = 16                      # per side of n

# key_0 with b_i = n - 1 and r_i = 2^31 (search_exit_eq; i = 4 and 8: the first half of a trip, 7: the second)
EXIT_EQ = {31: {
    7: (0x77269ddd8b45e59e,),
    8: (0x543fd88b8d60f46d, 0x37920b919135a436),
}, 21: {
    4: (0xc3865b441018170e,),
    7: (0x60a72d797e209edc, 0xdcbf6d08a2a280e4, 0x1a90852a2f9609c6, 0xd1c072dc25047cd2, 0xd6fd958d50d5ff2d, 0x9eb8f03ccbbcbbbd,
        0x0550ec764a5c8a62, 0x1e21be6fd775dba4),
    8: (0xa6ade04c8edc5980, 0xfb868f50de758f58, 0xd4ef3d58d2dd7bf7, 0x6a4f3b26fb4bbe07, 0x16f1422d7bb62241, 0xeed69432e4f589dc,
        0x2b453a7b6585c130, 0x4a2e84f1a935fc1f),
}}

SETTINGS = {
    "default": {},
    "cut1_pcut1": {"HULK_JUMP_CUT": "1", "HULK_JUMP_PCUT": "1"},
    "cut63_pcut1": {"HULK_JUMP_CUT": "63", "HULK_JUMP_PCUT": "1"},
    "cut0": {"HULK_JUMP_CUT": "0"},
    "regions_1": {"HULK_JUMP_REGIONS": "1"},
    "regions_3": {"HULK_JUMP_REGIONS": "3"},
    "regions_8": {"HULK_JUMP_REGIONS": "8"},
    "no_guard": {"HULK_JUMP_NO_GUARD": "1"},
}
REGIONS_OF = {"regions_1": 1, "regions_3": 3, "regions_8": 8}


# ---- the reference, in plain Python -----------------------------------------------------------------------------------------
def trace(key, n):
    """[(b_i, r_i, p_i)] of every step of the chain of `key`, the last one being the step that leaves (p >= n)"""
    out, b = [], 0
    while True:
        key = (key * A + 1) & M64
        r = (key >> 33) + 1
        p = float(b + 1) * (float(1 << 31) / float(r))
        out.append((b, r, p))
        if p >= n:
            return out
        b = int(p)


def jump_ref(key, n):
    return trace(key, n)[-1][0]


# ---- candidate search, numpy (the same doubles) --------------------------------------------------------------------------------
_A, _AINV, _ONE = np.uint64(A), np.uint64(A_INV), np.uint64(1)


def state_before(key0, n, i):
    """(alive, b_i): whether the chain of each key reaches step i, and its b there"""
    b = np.zeros(key0.shape, np.int64)
    alive = np.ones(key0.shape, bool)
    key = key0.copy()
    for _ in range(i):
        key = key * _A + _ONE
        r = (key >> np.uint64(33)) + _ONE
        p = (b + 1).astype(np.float64) * (float(1 << 31) / r.astype(np.float64))
        alive &= p < n
        b = np.where(alive, p.astype(np.int64), b)
    return alive, b


def key0_of(r, low, i):
    """key_0 of the keys whose step-i key is (r - 1) << 33 | low"""
    key = ((r - 1).astype(np.uint64) << np.uint64(33)) | low
    for _ in range(i + 1):
        key = (key - _ONE) * _AINV
    return key


def chain_lengths(key0, n):
    b = np.zeros(key0.shape, np.int64)
    steps = np.zeros(key0.shape, np.int64)
    idx = np.arange(key0.size)
    key = key0.copy()
    while idx.size:
        key = key * _A + _ONE
        r = (key >> np.uint64(33)) + _ONE
        p = (b[idx] + 1).astype(np.float64) * (float(1 << 31) / r.astype(np.float64))
        steps[idx] += 1
        go = p < n
        b[idx[go]] = p[go].astype(np.int64)
        idx, key = idx[go], key[go]
    return steps


def search_exit_eq(k, i, chunks, seed):
    """key_0 whose step-i product is n exactly: r_i = 2^31 and b_i = n - 1 (how EXIT_EQ was found; 2^22 candidates per chunk,
    about a second each — not run by the tests)"""
    n, rng, found = k ** 4, np.random.default_rng(seed), []
    for _ in range(chunks):
        low = rng.integers(0, 1 << 33, size=1 << 22, dtype=np.uint64)
        k0 = key0_of(np.full(low.size, 1 << 31, np.int64), low, i)
        alive, b = state_before(k0, n, i)
        found += [int(x) for x in k0[alive & (b == n - 1)]]
    return found


def build_cases(k):
    """name -> uint64 array of key_0; per-case preconditions are asserted in plain Python"""
    n = k ** 4
    rng = np.random.default_rng(1000 + k)
    c = {"random": rng.integers(0, 1 << 64, size=4096, dtype=np.uint64)}
    for i in STEPS:
        # exact-integer products, r_i = 2^j: Q = (b_i + 1) * 2^(31 - j)
        C = 1 << 13
        j = rng.integers(18, 32, size=C)
        low = rng.integers(0, 1 << 33, size=C, dtype=np.uint64)
        k0 = key0_of(np.int64(1) << j, low, i)
        alive, b = state_before(k0, n, i)
        pow2 = k0[alive & (((b + 1) << (31 - j)) < n)][:PER_STEP_EXACT // 2]
        # ... and r_i = o * 2^j, o odd > 1 dividing b_i + 1
        o = 2 * rng.integers(1, 16, size=C) + 1
        j = rng.integers(14, 27, size=C)                 # o * 2^j < 2^31
        low = rng.integers(0, 1 << 33, size=C, dtype=np.uint64)
        k0 = key0_of(o << j, low, i)
        alive, b = state_before(k0, n, i)
        odd = k0[alive & ((b + 1) % o == 0) & ((((b + 1) // o) << (31 - j)) < n)][:PER_STEP_EXACT // 2]
        c[f"exact_{i}"] = np.concatenate([pow2, odd])
        # exit decisions at n: r_i = floor((b_i + 1) * 2^31 / n) (the product is the nearest one >= n) or that plus 1 (below n).
        # b_i is guessed from the distribution random chains have at step i; a candidate counts if its own chain gets there
        alive, b = state_before(rng.integers(0, 1 << 64, size=1 << 16, dtype=np.uint64), n, i)
        C = 1 << (18 if i <= 4 else 21)
        bg = rng.choice(b[alive], size=C)
        side = rng.integers(0, 2, size=C)
        r = ((bg + 1) << 31) // n + side
        low = rng.integers(0, 1 << 33, size=C, dtype=np.uint64)
        ok = (r >= 1) & (r <= (1 << 31))
        k0 = key0_of(np.where(ok, r, 1), low, i)
        alive, b = state_before(k0, n, i)
        hit = ok & alive & (b == bg)
        c[f"exit_{i}"] = np.concatenate([k0[hit & (side == s)][:PER_STEP_EXIT] for s in (0, 1)])
    # chains of one step: r_0 <= 2^31 / n
    r0 = rng.integers(1, (1 << 31) // n + 1, size=64)
    c["one_step"] = key0_of(r0, rng.integers(0, 1 << 33, size=64, dtype=np.uint64), 0)
    # the longest chains among 10^6 random keys, and chains of every length up to 24: odd and even, an exit in either half
    many = rng.integers(0, 1 << 64, size=1_000_000, dtype=np.uint64)
    steps = chain_lengths(many, n)
    c["longest"] = many[np.argsort(steps)[-32:]]
    c["by_length"] = np.concatenate([many[steps == s][:8] for s in range(1, 25)])
    if k in EXIT_EQ:
        c["exit_eq"] = np.array([x for i in sorted(EXIT_EQ[k]) for x in EXIT_EQ[k][i]], dtype=np.uint64)
    return c


@pytest.fixture(scope="module")
def cases():
    return {k: build_cases(k) for k in KS}


def mixed(c):
    """every case of a k in one array, the constructed keys scattered among the random ones"""
    allk = np.concatenate([c[name] for name in sorted(c)])
    return allk[np.random.default_rng(7).permutation(allk.size)]


@pytest.fixture(scope="module")
def reference(cases):
    """{k: {key_0: bin}} for every key of every case, computed once"""
    return {k: {int(x): jump_ref(int(x), k ** 4) for x in mixed(c)} for k, c in cases.items()}


_RUNNER = """
import ctypes, sys
import numpy as np
sys.path.insert(0, {root!r})
import hulk_amd
from hulk_amd import _lib
L = _lib.load()
assert L.hulk_build_info().endswith(b" experiments=1")
vp = ctypes.c_void_p
L.hulk_debug_jump.restype = ctypes.c_int
L.hulk_debug_jump.argtypes = [vp, vp, ctypes.c_uint64, ctypes.c_uint32, vp, vp]
d = np.load(sys.argv[1])
out = {{}}
for k in {ks!r}:
    g = hulk_amd.GpuSketcher(k, 9, 16, 0)
    for name in d.files:
        if not name.startswith("k%d_" % k):
            continue
        vals = np.ascontiguousarray(d[name])
        lens = {lens!r} if name.endswith("_mixed") else (449,)
        for rl in lens:
            bins = np.zeros(vals.size, np.uint32)
            hits = ctypes.c_uint64(0)
            rc = L.hulk_debug_jump(g._ctx, vals.ctypes.data, vals.size, rl, bins.ctypes.data, ctypes.byref(hits))
            assert rc == 0, (name, rl, rc)
            out["%s_len%d" % (name, rl)] = bins
            out["%s_len%d_hits" % (name, rl)] = np.uint64(hits.value)
    g.close()
np.savez(sys.argv[2], **out)
print("DONE", flush=True)
"""


@pytest.fixture(scope="module")
def gpu_runs(cases, tmp_path_factory):
    """{setting: {"k<k>_<case>_len<region_len>": bins, "..._hits": guarded lane-steps}}: one child process per setting; the
    single cases run at region length 449 in the default and the no-guard settings, the mixed array at every length everywhere"""
    assert os.path.exists(EXP_LIB), "profiling build (libhulkhip_exp.so) not built"
    d = tmp_path_factory.mktemp("jump_pair")
    arrays, only_mixed = {}, {}
    for k, c in cases.items():
        only_mixed[f"k{k}_mixed"] = mixed(c)
        for name, vals in c.items():
            arrays[f"k{k}_{name}"] = vals
    arrays.update(only_mixed)
    np.savez(str(d / "in_all.npz"), **arrays)
    np.savez(str(d / "in_mixed.npz"), **only_mixed)
    env0 = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    out = {}
    for setting, env in SETTINGS.items():
        src = "in_all.npz" if setting in ("default", "no_guard") else "in_mixed.npz"
        dst = str(d / f"out_{setting}.npz")
        r = subprocess.run([sys.executable, "-c", _RUNNER.format(root=ROOT, ks=KS, lens=REGION_LENS), str(d / src), dst],
                           env=dict(env0, HULK_LIB="exp", **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "DONE" in r.stdout, f"{setting}: {r.stderr[-2000:]}"
        out[setting] = dict(np.load(dst))
    return out


def want(reference, k, keys):
    return np.array([reference[k][int(x)] for x in keys], dtype=np.uint32)


# ---- the cases are what they say (no GPU result involved) ---------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_constructed_cases_hold_their_preconditions(cases, k):
    n, c = k ** 4, cases[k]
    for i in STEPS:
        keys = c[f"exact_{i}"]
        assert keys.size == PER_STEP_EXACT, (i, keys.size)
        pow2 = 0
        for x in keys:
            tr = trace(int(x), n)
            assert len(tr) > i, "the chain ends before step i"
            b, r, _ = tr[i]
            assert ((b + 1) << 31) % r == 0 and ((b + 1) << 31) // r < n
            pow2 += r & (r - 1) == 0
            assert r & (r - 1) == 0 or (r >> ((r & -r).bit_length() - 1)) > 1
        assert pow2 == PER_STEP_EXACT // 2, (i, pow2)
        keys = c[f"exit_{i}"]
        assert keys.size == 2 * PER_STEP_EXIT, (i, keys.size)
        leave = 0
        for x in keys:
            tr = trace(int(x), n)
            assert len(tr) > i
            b, r, p = tr[i]
            f = ((b + 1) << 31) // n
            assert r in (f, f + 1)
            assert (p >= n) == (r == f)                  # floor: the nearest quotient at or above n; plus 1: the nearest below
            leave += r == f
        assert leave == PER_STEP_EXIT
    for i, keys in EXIT_EQ.get(k, {}).items():              # Q = n exactly: the step leaves, with the double n itself
        for x in keys:
            tr = trace(x, n)
            assert len(tr) == i + 1
            b, r, p = tr[i]
            assert ((b + 1) << 31) == r * n and p == n and b == n - 1 and r == 1 << 31
    for x in c["one_step"]:
        tr = trace(int(x), n)
        assert len(tr) == 1 and tr[0][1] <= (1 << 31) // n
    longest = [len(trace(int(x), n)) for x in c["longest"]]
    print("longest chains:", sorted(longest)[-4:])
    assert max(longest) >= 28
    lengths = {len(trace(int(x), n)) for x in c["by_length"]}
    assert set(range(1, 21)) <= lengths                   # odd and even


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_random_values(gpu_runs, cases, reference, k):
    got = gpu_runs["default"]
    keys = cases[k]["random"]
    assert np.array_equal(got[f"k{k}_random_len449"], want(reference, k, keys))
    hits = int(got[f"k{k}_random_len449_hits"])
    print("guarded lane-steps over 4096 random values:", hits)
    assert hits <= 2                                      # expected 4096 * 12.8 * 2^-19 = 0.1


@pytest.mark.parametrize("i", STEPS)
@pytest.mark.parametrize("k", KS)
def test_exact_integer_products(gpu_runs, cases, reference, k, i):
    got = gpu_runs["default"]
    keys = cases[k][f"exact_{i}"]
    assert np.array_equal(got[f"k{k}_exact_{i}_len449"], want(reference, k, keys))
    assert int(got[f"k{k}_exact_{i}_len449_hits"]) >= keys.size


@pytest.mark.parametrize("name", [f"exit_{i}" for i in STEPS] + ["one_step", "longest", "by_length"])
@pytest.mark.parametrize("k", KS)
def test_exit_decisions_and_chain_lengths(gpu_runs, cases, reference, k, name):
    got = gpu_runs["default"][f"k{k}_{name}_len449"]
    assert np.array_equal(got, want(reference, k, cases[k][name]))


@pytest.mark.parametrize("k", KS)
def test_product_equal_to_n(gpu_runs, cases, reference, k):
    """Q = n exactly: the bin is n - 1 either way, so the guard counter is the check — one exact step per key at least"""
    keys = cases[k]["exit_eq"]
    assert keys.size == sum(len(v) for v in EXIT_EQ[k].values()) and {7, 8} <= set(EXIT_EQ[k])     # both halves of a trip
    exp = want(reference, k, keys)
    assert np.all(exp == k ** 4 - 1)
    assert np.array_equal(gpu_runs["default"][f"k{k}_exit_eq_len449"], exp)
    hits = int(gpu_runs["default"][f"k{k}_exit_eq_len449_hits"])
    print("guarded lane-steps over", keys.size, "keys with Q = n:", hits)
    assert hits >= keys.size
    assert np.array_equal(gpu_runs["no_guard"][f"k{k}_exit_eq_len449"], exp)
    assert int(gpu_runs["no_guard"][f"k{k}_exit_eq_len449_hits"]) == 0


@pytest.mark.parametrize("setting", [s for s in SETTINGS if s != "no_guard"])
@pytest.mark.parametrize("k", KS)
def test_region_shapes_and_pool_settings(gpu_runs, cases, reference, k, setting):
    keys = mixed(cases[k])
    exp = want(reference, k, keys)
    n_exact = sum(cases[k][f"exact_{i}"].size for i in STEPS) + (cases[k]["exit_eq"].size if "exit_eq" in cases[k] else 0)
    if setting in REGIONS_OF:                             # a region count that is no multiple of R
        assert any(-(-keys.size // rl) % REGIONS_OF[setting] for rl in REGION_LENS) or REGIONS_OF[setting] == 1
    for rl in REGION_LENS:
        got = gpu_runs[setting][f"k{k}_mixed_len{rl}"]
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (rl, bad.size, [hex(int(x)) for x in keys[bad[:4]]])
        assert int(gpu_runs[setting][f"k{k}_mixed_len{rl}_hits"]) >= n_exact, rl


def test_without_the_guard_an_exact_product_goes_wrong(gpu_runs, cases, reference):
    """teeth: HULK_JUMP_NO_GUARD leaves the integer quotients to the shared reciprocal's rounding"""
    wrong = 0
    for k in KS:
        for i in STEPS:
            keys = cases[k][f"exact_{i}"]
            got = gpu_runs["no_guard"][f"k{k}_exact_{i}_len449"]
            assert int(gpu_runs["no_guard"][f"k{k}_exact_{i}_len449_hits"]) == 0
            wrong += int((got != want(reference, k, keys)).sum())
    print("exact-integer cases that differ without the guard:", wrong, "of", 2 * len(STEPS) * PER_STEP_EXACT)
    assert wrong >= 1
