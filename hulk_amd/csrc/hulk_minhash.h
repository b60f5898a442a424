// hulk_minhash.h — device side of the two MinHash sketches (reference: src/minhash/kmv.go:39-71, khf.go:34-45), shared by
// hulk_minhash.hip (the kernels that read a minimizer list or a long sequence's set table) and hulk_minimizer.hip (the hook in
// k_minimizer_bin's queue drain).  wave64 code for CDNA4; plain C++ and vector memory operations only.
//
// KMV.  kmv[S] starts as MaxUint64 everywhere.  AddHash(v) is a "bubble": for i = 0 .. S-1 { old = atomicMin(&kmv[i], v);
// v = max(old, v) } — each step either leaves both alone or swaps the carried value with the entry, so the multiset
// (entries + carried values) never changes, and what falls off the end is dropped.  A carried value passes entry i only
// once kmv[i] <= it, and entries only ever fall, so at rest every entry is <= every dropped value: the entries are the S
// smallest of the fed MULTISET (duplicates kept, kmv.go has no de-duplication), whatever the order and however many
// waves, work lanes or kernels insert at once.  By the same argument kmv[S-1] is at all times >= every other entry, so a
// value >= kmv[S-1] would walk the whole array without a swap: the feed skips it (strict '<' is exactly "this AddHash is a
// no-op"; a stale, larger reading of kmv[S-1] only lets a no-op through).  A step whose entry was read as <= v is skipped
// the same way.  After warm-up the cost per value is that one compare.
//
// KHF.  khf[i] = min over fed x of (x + i*x) mod 2^64.  MH_KHF_MIN: no product can wrap (2k + 8 + ceil(log2 S) <= 64), the
// products are monotone in x, and the signature is (i+1) * min(x): the feed is one min-reduction into *xmin.  MH_KHF_BRUTE:
// every value updates every slot; lane l owns slots l, l+64, ..., the next owned slot's product is a 64-bit add of 64*x.
#pragma once
#include "hulk_device.h"

namespace hulk {
namespace {

__device__ __forceinline__ uint64_t mh_readlane(uint64_t v, int l) {   // l wave-uniform
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ unsigned long long mh_load(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t mh_wave_min(uint64_t v) {
    for (int off = 32; off; off >>= 1) { const uint64_t o = __shfl_xor(v, off); v = o < v ? o : v; }
    return v;
}

// KMVsketch.AddHash(v) by the whole wave; v is wave-uniform
__device__ __noinline__ void kmv_insert_wave(unsigned long long *a, uint32_t S, uint64_t v) {
    const int lane = lane_id();
    for (uint32_t base = 0; base < S; base += 64) {
        const uint32_t idx = base + (uint32_t)lane;
        const uint64_t cur = idx < S ? mh_load(a + idx) : 0ull;        // (0: never above the carried value)
        uint64_t m = __ballot(cur > v);
        while (m) {
            const int i = __builtin_ctzll(m);
            unsigned long long old = 0;
            if (lane == i) old = atomicMin(a + base + i, (unsigned long long)v);
            old = mh_readlane(old, i);
            if (old > v) v = old;                                       // swapped: carry the entry on
            m = __ballot(cur > v) & ~(i == 63 ? ~0ull : ((2ull << i) - 1ull));
        }
        if (v == ~0ull) return;                                         // nothing is above MaxUint64: the rest are no-ops
    }
}

// the values of one wave (x where `active`) into the sketches the context keeps; `run_min` is the lane's running minimum for
// MH_KHF_MIN (reduced and published once, by mh_finish_wave)
__device__ __forceinline__ void mh_feed_wave(const MinHashState &M, uint64_t x, bool active, uint64_t &run_min) {
    const int lane = lane_id();
    if (M.mode & MH_KMV) {
        const unsigned long long *tau = M.kmv + (M.S - 1);
        uint64_t c = __ballot(active && x < mh_load(tau));
        while (c) {
            const int j = __builtin_ctzll(c);
            c &= c - 1;
            const uint64_t v = mh_readlane(x, j);
            if (v < mh_load(tau)) kmv_insert_wave(M.kmv, M.S, v);       // (the bound may have fallen since the ballot)
        }
    }
    if (M.mode & MH_KHF_MIN) { if (active && x < run_min) run_min = x; }
    if (M.mode & MH_KHF_BRUTE) {
        uint64_t c = __ballot(active);
        while (c) {
            const int j = __builtin_ctzll(c);
            c &= c - 1;
            const uint64_t xs = mh_readlane(x, j), step = xs << 6;
            uint64_t val = xs * (uint64_t)(lane + 1);
            for (uint32_t slot = (uint32_t)lane; slot < M.S; slot += 64) {
                // (entries only fall: a stale reading is a larger one and merely lets a no-op atomic through)
                if (val < M.khf[slot]) atomicMin(M.khf + slot, (unsigned long long)val);
                val += step;
            }
        }
    }
}
__device__ __forceinline__ void mh_finish_wave(const MinHashState &M, uint64_t run_min) {
    if (M.mode & MH_KHF_MIN) {
        const uint64_t m = mh_wave_min(run_min);
        if (lane_id() == 0 && m < mh_load(M.xmin)) atomicMin(M.xmin, (unsigned long long)m);
    }
}

}  // namespace
}  // namespace hulk
