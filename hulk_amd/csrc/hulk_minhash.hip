// hulk_minhash.hip — the KMV (bottom-k) and KHF (k-hash-functions) MinHash sketches of a context created with
// HULK_FLAG_KMV / HULK_FLAG_KHF, fed with what the boss's collector feeds the k-mer spectrum (src/pipeline/boss.go:90-95):
// every read's distinct minimizers once.  Reference semantics: src/minhash/kmv.go:39-71, khf.go:34-55; how they are kept
// exact under any order and concurrency: hulk_minhash.h.
//   k_mh_scan<NS, false>  short reads: the per-wave minimizer list k_minimizer_fast wrote (MinimizerList.x / cnt)
//   k_mh_scan<NS, true>   long sequences: the set tables k_long_tile left behind — a sequence's distinct minimizers are
//                         exactly the occupied entries of its table, so the long-sequence kernels themselves are untouched
//   (the generic kernel k_minimizer_bin<true> feeds from its own queue drain: hulk_minimizer.hip)
//   k_mh_merge            MinHash.Merge of a signature handed in by the host
// All kernels are wave64 code for CDNA4; none of them has a CPU or library fallback.
#include "hulk_minhash.h"

namespace hulk {
namespace {

// NS = owned KHF slots per lane of the brute-force path (64 * NS >= S), 0 = no brute-force KHF in this launch.
// A wave takes 64 values at a time (one per lane), compares them with the KMV bound, and — brute force — walks them one by
// one, wave-uniformly, over the slot minima it keeps in registers; those are folded into khf[] once, at the end.
template <int NS, bool TABLE>
__global__ __launch_bounds__(256) void k_mh_scan(const uint64_t *__restrict__ vals, const uint32_t *__restrict__ cnt,
                                                 uint64_t rcap, uint64_t n_units, MinHashState M) {
    const int lane = lane_id();
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t part[NS > 0 ? NS : 1];
#pragma unroll
    for (int t = 0; t < (NS > 0 ? NS : 1); t++) part[t] = ~0ull;
    uint64_t run_min = ~0ull;
    unsigned long long nfed = 0;                                        // wave-uniform
    const unsigned long long *tau_p = M.kmv + (M.S - 1);
    uint64_t tau = (M.mode & MH_KMV) ? mh_load(tau_p) : 0ull;
    // a unit = a region of the list (rcap entries, cnt[] of them filled) or 64 consecutive entries of the table
    const uint64_t gw = (uint64_t)blockIdx.x * 4 + wid, stride = (uint64_t)gridDim.x * 4;
    for (uint64_t u = gw; u < n_units; u += stride) {
        uint32_t n = 64;
        const uint64_t *src = vals + (TABLE ? u * 64 : u * rcap);
        if (!TABLE) { n = __builtin_amdgcn_readfirstlane(cnt[u]); if (n > rcap) n = (uint32_t)rcap; }
        for (uint32_t i0 = 0; i0 < n; i0 += 64) {
            bool active = i0 + (uint32_t)lane < n;
            uint64_t x = active ? src[i0 + lane] : ~0ull;
            if (TABLE) active = x != TAB_EMPTY;
            const uint64_t am = __ballot(active);
            nfed += (unsigned long long)__popcll(am);
            if (M.mode & MH_KMV) {
                uint64_t c = __ballot(active && x < tau);
                if (c) {
                    while (c) {
                        const int j = __builtin_ctzll(c);
                        c &= c - 1;
                        const uint64_t v = mh_readlane(x, j);
                        if (v < mh_load(tau_p)) kmv_insert_wave(M.kmv, M.S, v);
                    }
                    tau = mh_load(tau_p);
                }
            }
            if (M.mode & MH_KHF_MIN) { if (active && x < run_min) run_min = x; }
            if (NS > 0) {
                uint64_t c = am;
                while (c) {
                    const int j = __builtin_ctzll(c);
                    c &= c - 1;
                    const uint64_t xs = mh_readlane(x, j), step = xs << 6;
                    uint64_t val = xs * (uint64_t)(lane + 1);
#pragma unroll
                    for (int t = 0; t < NS; t++) {
                        // (64-bit unsigned minimum by compare and select: the products cover all 64 bits, so v_min_f64 on the
                        //  integer keys — valid for the minimizer values themselves at k <= 27 — is not)
                        part[t] = val < part[t] ? val : part[t];
                        val += step;
                    }
                }
            }
        }
    }
    mh_finish_wave(M, run_min);
    if (NS > 0) {
#pragma unroll
        for (int t = 0; t < NS; t++) {
            const uint32_t slot = (uint32_t)lane + 64u * (uint32_t)t;
            if (slot < M.S && part[t] < mh_load(M.khf + slot)) atomicMin(M.khf + slot, (unsigned long long)part[t]);
        }
    }
    __shared__ unsigned long long blk_fed[4];
    if (lane == 0) blk_fed[wid] = nfed;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = blk_fed[0] + blk_fed[1] + blk_fed[2] + blk_fed[3];
        if (t) atomicAdd(&M.fed[blockIdx.x & (MH_FED_SLOTS - 1)], t);
    }
}

// MinHash.Merge (khf.go:49-55; KMV: the other sketch's values fed into this one): one wave
__global__ __launch_bounds__(64) void k_mh_merge(const uint64_t *__restrict__ vals, uint32_t n, int khf, MinHashState M) {
    const int lane = lane_id();
    if (khf) {
        for (uint32_t i = (uint32_t)lane; i < n && i < M.S; i += 64) atomicMin(M.khf + i, (unsigned long long)vals[i]);
        return;
    }
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const bool active = i0 + (uint32_t)lane < n;
        const uint64_t x = active ? vals[i0 + lane] : ~0ull;
        uint64_t c = __ballot(active);
        while (c) {
            const int j = __builtin_ctzll(c);
            c &= c - 1;
            kmv_insert_wave(M.kmv, M.S, mh_readlane(x, j));
        }
    }
}

template <bool TABLE>
hipError_t launch_scan(hipStream_t s, const uint64_t *vals, const uint32_t *cnt, uint64_t rcap, uint64_t n_units,
                       const MinHashState &M) {
    if (!M.mode || !n_units) return hipSuccess;
    // enough waves to fill the chip, few enough that the folds at the end (one guarded atomic per slot and wave) stay small
    uint64_t blocks = (n_units + 3) / 4;
    if (blocks > 2048) blocks = 2048;
    const dim3 g((unsigned)blocks), b(256);
    prof_mark(s, TABLE ? "k_mh_scan_table" : "k_mh_scan_list");
#define HULK_MH_LAUNCH(NSv) hipLaunchKernelGGL((k_mh_scan<NSv, TABLE>), g, b, 0, s, vals, cnt, rcap, n_units, M)
    if (!(M.mode & MH_KHF_BRUTE)) HULK_MH_LAUNCH(0);
    else if (M.S <= 64) HULK_MH_LAUNCH(1);
    else if (M.S <= 128) HULK_MH_LAUNCH(2);
    else if (M.S <= 256) HULK_MH_LAUNCH(4);
    else if (M.S <= 512) HULK_MH_LAUNCH(8);
    else if (M.S <= 1024) HULK_MH_LAUNCH(16);
    else if (M.S <= 2048) HULK_MH_LAUNCH(32);
    else if (M.S <= MH_MAX_SKETCH) HULK_MH_LAUNCH(64);
    else return hipErrorInvalidValue;
#undef HULK_MH_LAUNCH
    return hipGetLastError();
}

}  // namespace

hipError_t launch_minhash_list(hipStream_t s, const MinimizerList &ml, uint64_t n_reads, const MinHashState &M) {
    const uint64_t regions = (n_reads + FAST_READS_PER_WAVE - 1) / FAST_READS_PER_WAVE;
    return launch_scan<false>(s, ml.x, ml.cnt, ml.rcap, regions, M);
}

// table_total is a sum of powers of two >= 1024 (one slice per long sequence): a multiple of 64
hipError_t launch_minhash_table(hipStream_t s, const uint64_t *d_table, uint64_t table_total, const MinHashState &M) {
    return launch_scan<true>(s, d_table, nullptr, 0, table_total / 64, M);
}

hipError_t launch_minhash_merge(hipStream_t s, const uint64_t *d_vals, uint32_t n, int khf, const MinHashState &M) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_mh_merge, dim3(1), dim3(64), 0, s, d_vals, n, khf, M);
    return hipGetLastError();
}

}  // namespace hulk
