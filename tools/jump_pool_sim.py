#!/usr/bin/env python3
"""Prices the ways k_jump_bin can deal with the slow chains of a round, on the CPU, with the real hash (pure numpy, no GPU).

A wave runs 64 jump-hash chains in lock step; a chain takes 12.75 +- 3.3 steps at n = 21^4, so the last lanes of a round keep
the whole wave issuing.  The model counts wave-steps (one trip of the step loop for the whole wave, whatever the number of live
lanes) and rounds per 64 values for
  * `left`: a round ends when <= cut lanes are live, the leftovers of a region (at most 64) are finished by a second kernel in
    one wave, to the last one (the scheme until round 6: cut 10 + k_jump_left);
  * `pool`: a wave owns R regions; a round ends when <= cut lanes are live, the leftovers go to a 64-entry pool of the wave; a
    pool that would pass 64 is filled to 64 and run as a dense round until <= pcut are live; the pool is drained at the wave's end.
Cost model, counted in k_jump_bin's gfx950 assembly (tests/test_k1b_lean.py compiles it): 17 instructions per wave-step (14
VALU + the exit test) and, outside the step loop, in VALU instructions
  * 11 per main round (index, prefetch address, t = 0, bucket -> word, store address, next value into the loop's registers),
  * 10 per hand-over (two mbcnt, destination = select on the scalar mask, four conditional receives) + four ds_permute_b32,
  * 12 per pool round (t from the word and back, store address, compaction's destination) + four ds_permute_b32,
  *  5 more when the pool wraps (the mask of the chains that still fit; the round's key set aside and brought back).
Scalar instructions and loads are not priced.  profiles/k1b_lean.md sets the measured counters beside the model: outside the
loop, per 64 values, 38.4 VALU + 8.3 ds_permute_b32 = 46.7 measured at cut 24 / pcut 32 / R 4 against 44.5 modelled, and 54.8
against 52.2 at cut 32 (the difference is the per-region set-up, which is not modelled).
The `left` scheme is history (its second kernel is gone); its rounds are priced like main rounds and its hand-over like a push.

    python tools/jump_pool_sim.py [--keys 1300000] [--bins 194481] [--region 432]
"""
import argparse

import numpy as np

STEP_INSTR = 17
ROUND_VALU, PUSH_VALU, POOL_ROUND_VALU, WRAP_VALU, PERMUTES = 11, 10, 12, 5, 4


def chain_lengths(keys, n):
    """steps of go-jump's loop per key: b = j until j >= n, j = int64(float64(b + 1) * (float64(1 << 31) / float64((key >> 33) + 1)))"""
    key = keys.copy()
    t = np.zeros(len(keys))
    steps = np.zeros(len(keys), dtype=np.int32)
    live = np.ones(len(keys), dtype=bool)
    a = np.uint64(2862933555777941757)
    with np.errstate(over="ignore"):
        while live.any():
            key[live] = key[live] * a + np.uint64(1)
            q = 2147483648.0 / ((key[live] >> np.uint64(33)).astype(np.float64) + 1.0)
            p = (t[live] + 1.0) * q
            steps[live] += 1
            done = p >= n
            idx = np.flatnonzero(live)
            t[idx[~done]] = np.trunc(p[~done])
            live[idx[done]] = False
    return steps


def run_round(rem, cut):
    """one lock-step round over the remaining chain lengths `rem`: (wave-steps, lengths still to go of the <= cut survivors)"""
    if len(rem) == 0:
        return 0, rem
    s = np.sort(rem)[::-1]
    steps = max(1, int(s[cut])) if cut < len(s) else 1        # the loop tests after a step: at least one
    left = rem[rem > steps] - steps
    return steps, left


def rounds_of(region):
    for i in range(0, len(region), 64):
        yield region[i:i + 64]                                 # lane l takes values l, l + 64, ...: a round is 64 consecutive values


def sim_left(regions, cut):
    """-> (wave-steps, rounds, instructions outside the step loop)"""
    wsteps = rounds = outside = 0
    for reg in regions:
        lo = []
        for r in rounds_of(reg):
            s, left = run_round(r, cut)
            wsteps += s; rounds += 1; outside += ROUND_VALU
            room = 64 - sum(map(len, lo))
            if len(left) > room:                               # the hand-over area is full: finished in place
                wsteps += int(left[room:].max()); left = left[:room]
            if len(left):
                outside += PUSH_VALU
            lo.append(left)
        lo = np.concatenate(lo) if lo else np.zeros(0, dtype=np.int32)
        if cut and len(lo):
            wsteps += int(lo.max()); rounds += 1; outside += ROUND_VALU
    return wsteps, rounds, outside


def sim_pool(regions, cut, pcut, R):
    """-> (wave-steps, rounds, instructions outside the step loop: VALU + ds_permute_b32)"""
    wsteps = rounds = outside = 0
    push, pool_round = PUSH_VALU + PERMUTES, POOL_ROUND_VALU + PERMUTES
    for w in range(0, len(regions), R):
        pool = np.zeros(0, dtype=np.int32)
        for reg in regions[w:w + R]:
            for r in rounds_of(reg):
                s, left = run_round(r, cut)
                wsteps += s; rounds += 1; outside += ROUND_VALU
                if len(left) == 0:
                    continue
                if len(pool) + len(left) > 64:
                    room = 64 - len(pool)
                    outside += WRAP_VALU + (push if room else 0) + pool_round
                    s, pool = run_round(np.concatenate([pool, left[:room]]), pcut)
                    wsteps += s; rounds += 1
                    left = left[room:]
                outside += push
                pool = np.concatenate([pool, left])
        if len(pool):
            wsteps += int(pool.max()); rounds += 1; outside += pool_round
    return wsteps, rounds, outside


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keys", type=int, default=1300000)
    ap.add_argument("--bins", type=int, default=21 ** 4)
    ap.add_argument("--region", type=int, default=432, help="values per region (16 reads of 150 bp at w = 9: ~27 each)")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    keys = rng.integers(0, 2 ** 64, size=a.keys, dtype=np.uint64)
    L = chain_lengths(keys, float(a.bins))
    print(f"chain: {L.mean():.2f} +- {L.std():.2f} steps, max {L.max()}")
    regions = [L[i:i + a.region] for i in range(0, len(L), a.region)]
    per64 = len(L) / 64.0

    def row(name, ws, rd, outside):
        print(f"{name:34s} {ws / per64:7.2f} {rd / per64:7.2f} {outside / per64:8.1f} {(ws * STEP_INSTR + outside) / per64:8.0f}")
    print(f"{'scheme':34s} {'wsteps':>7s} {'rounds':>7s} {'outside':>8s} {'instr':>8s}   (per 64 values)")
    row("every round to its end (cut 0)", *sim_left(regions, 0))
    row("cut 10 + second kernel", *sim_left(regions, 10))
    for R in (1, 2, 4, 8):
        for cut in (16, 24, 32, 40):
            for pcut in (16, 32):
                if cut + pcut <= 64:
                    row(f"pool R={R} cut={cut} pcut={pcut}", *sim_pool(regions, cut, pcut, R))


if __name__ == "__main__":
    main()
