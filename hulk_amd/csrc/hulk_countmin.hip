// hulk_countmin.hip — KmerSpectrum.Cardinality and count-min Add() for a batch of spectra, bin order.
//   K2  k_count_used       the 1 % rule (kmerspectrum.go:53-55,84-96)
//   K3  k_cms_segsum/k_cms_base/k_cms_freq   src/countmin/countmin.go:103-147
//       k_cms_steady_sums/k_cms_steady_add   what is left of K3 in a flush the host knows k_flush_decide passes over:
//                          the batch's spectra summed per bin, then one count-min pass
//       k_elem_*/k_cmsd_*  the same with uniform scaling (0 < decay < 1)
// The replay (k_*_freq) is a 2 x 2 over one skeleton, cms_replay<order>(arithmetic):
//                         LDS order (default)       chain order (fallback)
//   integer counters      k_cms_freq                k_cms_freq_chain
//   fp64 with decay       k_cmsd_freq               k_cmsd_freq_chain
// Three kernels rest on the LDS applying same-address lanes of one returning atomic in ascending lane order (k_lds_order_probe
// checks it on the device): the two LDS-order forms, for their results, and k_cmsd_segsum, for the reproducible order of its sums.
#include "hulk_device.h"

#include <math.h>
#include <stdlib.h>
#include <stdio.h>
#include <algorithm>
#include <mutex>

namespace hulk {
namespace {

// K2: number of used bins (bitvector PopCount in the reference).  grid = (blocks, count)
__global__ __launch_bounds__(256) void k_count_used(const uint32_t *__restrict__ hists, DevState *st,
                                                    FlushBatch fb) {
    __shared__ unsigned red[4];
    const int t = blockIdx.y;
    const uint32_t slot = ring_slot(fb, t);
    if (blockIdx.x == 0 && t == 0 && threadIdx.x < RING_MAX) st->used[fb.parity ^ 1][threadIdx.x] = 0;  // arm the next flush
    const uint32_t *hist = hists + (size_t)slot * (size_t)fb.num_bins;
    unsigned cnt = 0;
    for (int32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < fb.num_bins; b += gridDim.x * blockDim.x)
        cnt += hist[b] != 0;
    for (int off = 32; off; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane_id() == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt = red[0] + red[1] + red[2] + red[3];
        if (cnt) atomicAdd(&st->used[fb.parity][slot], cnt);   // one per block; the grid is small
    }
}

// ------------------------------------------------------------------------------------------
// K3 (no decay), bin-order form.  (Kernels that followed each counter's chain of bins, ~2000 apart, came first and are gone:
// they gathered 4-byte values along the chains, and rocprofv3 showed 13x more HBM traffic than the algorithmic bytes.)
// Every array is read in BIN order (coalesced) and the 7 x 2000 running counters live in LDS:
//   k_cms_segsum : per (spectrum, row, bin segment) sums per counter            (LDS atomics)
//   k_cms_base   : counter value in front of every (spectrum, segment)          (tiny prefix kernel)
//   k_cms_freq   : one workgroup per (segment, spectrum) replays the segment in bin order from there ("The replay" below)
// ------------------------------------------------------------------------------------------
constexpr int CMS_SEGS = 16;          // bin segments per spectrum
inline int cms_seg_chunks(int32_t num_bins) { return ((num_bins + 63) / 64 + CMS_SEGS - 1) / CMS_SEGS; }   // chunks of 64 bins per segment

// The row sums of one bin segment (k_cms_segsum, k_shard_local): the [depth][width] LDS counters start at zero and wave d < depth
// adds the counts of the segment's bins, from b0 on, to row d.  The caller's barrier comes before the counters are read.
__device__ __forceinline__ void cms_seg_row_sums(uint32_t *lctr, const uint32_t *__restrict__ hist, const uint16_t *__restrict__ pos16,
                                                 size_t B, int64_t b0, int depth, int width, int seg_chunks) {
    const int tid = threadIdx.x, lane = tid & 63, d = tid >> 6;
    for (int i = tid; i < depth * width; i += blockDim.x) lctr[i] = 0;
    __syncthreads();
    if (d >= depth) return;
    const uint16_t *pd = pos16 + (size_t)d * B;
    for (int c0 = 0; c0 < seg_chunks; c0 += 8) {                  // 8 chunks of loads in flight
        uint32_t h[8]; uint32_t p[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int64_t b = b0 + (int64_t)(c0 + u) * 64 + lane;
            const bool ok = (c0 + u < seg_chunks) && b < (int64_t)B;
            h[u] = ok ? hist[b] : 0u; p[u] = ok ? pd[b] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) if (h[u]) atomicAdd(&lctr[d * width + p[u]], h[u]);
    }
}

// Workgroup (segment, spectrum): the segment's row sums to segsum[t][d][seg][p].  STEADY (k_cms_steady_segsum, "The steady
// flush" below): the sums are all the count-min still needs of the spectrum, so the workgroup also wipes its segment — what
// cms_replay does for a batch k_flush_decide passed over — and touches nothing when the device-side proof is missing.
template <bool STEADY, class Hist>
__device__ __forceinline__ void cms_segsum(Hist *__restrict__ hists, const uint16_t *__restrict__ pos16,
                                           uint32_t *__restrict__ segsum, int depth, int width, int seg_chunks,
                                           const DevState *st, const FlushBatch &fb) {
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *lctr = (uint32_t *)smem;                           // [depth][width]
    const int seg = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const uint32_t gomask = batch_gomask(st, fb);
    if (!((gomask >> t) & 1u)) return;
    if (STEADY && !st->skip_exact[fb.parity]) return;            // (k_cms_steady_segadd raises the error)
    const size_t B = (size_t)fb.num_bins;
    Hist *hist = hists + (size_t)ring_slot(fb, t) * B;
    const int64_t b0 = (int64_t)seg * seg_chunks * 64;
    cms_seg_row_sums(lctr, hist, pos16, B, b0, depth, width, seg_chunks);
    __syncthreads();
    uint32_t *out = segsum + (((size_t)t * depth) * CMS_SEGS + 0) * width;
    for (int i = tid; i < depth * width; i += blockDim.x) {
        const int dd = i / width, p = i - dd * width;
        out[((size_t)dd * CMS_SEGS + seg) * width + p] = lctr[i];
    }
    if constexpr (STEADY) {
        const int64_t w1 = b0 + (int64_t)seg_chunks * 64;
        for (int64_t b = b0 + tid; b < w1 && b < (int64_t)B; b += blockDim.x) hist[b] = 0;      // Wipe (kmerspectrum.go:58-64)
    }
}
__global__ __launch_bounds__(512) void k_cms_segsum(const uint32_t *__restrict__ hists,
                                                    const uint16_t *__restrict__ pos16,
                                                    uint32_t *__restrict__ segsum, int depth, int width,
                                                    int seg_chunks, const DevState *st, FlushBatch fb) {
    cms_segsum<false>(hists, pos16, segsum, depth, width, seg_chunks, st, fb);
}

// ------------------------------------------------------------------------------------------
// The steady flush.  Once k_flush_decide has passed over a whole batch of a context without decay, it passes over every later
// one: the counters only grow, so their minimum m only grows; kminslot is static; the weights change only in a batch that was
// evaluated; hence bound = kminslot / m rises towards 0 while every threshold stays where it is.  The host learns the verdict
// from the word k_flush_decide stores to its memory (hulk_flush.hip, steady_adopt) and from then on queues, behind k_count_used
// and k_flush_decide, only what such a batch still changes: the counters (countmin.go:122-127), the element count and the
// 1 % rule (kmerspectrum.go:84-96), and the wipe (kmerspectrum.go:58-64).
// Nothing reads an estimate in such a flush and the counters are integers, so the spectra of the batch need not be told
// apart: counters += CM(sum over the spectra that go), one count-min pass over ONE summed spectrum.
//   k_cms_steady_sums : thread per bin, hsum[b] = the 64-bit sum of bin b over the spectra that go; wipes those spectra
//   k_cms_steady_add  : workgroup per (bin segment, row, part of the row): hsum into at most 8 KB of 64-bit LDS counters, the
//                       non-zero ones into ctr with global 64-bit atomics (integer adds commute); thread 0 keeps the books
// Every width from hsum to ctr is 64 bits: a sum spans up to RING_MAX spectra and a whole bin segment.
// k_flush_decide still runs in front of them and stays the proof on the device: without skip_exact neither kernel changes
// anything and the batch ends in HULK_ERR_STATE — lost loudly.  No `base`, no replay workgroups with 112 KB of LDS, no scan,
// no LDS request that does not fit beside six k_minimizer_fast workgroups.
// HULK_STEADY_SEGSUM (profiling build): the form in front of this one, per-(spectrum, segment) row sums in 56 KB of LDS
// (k_cms_steady_segsum / k_cms_steady_segadd), under the same two marks — the A/B in one process image.
// ------------------------------------------------------------------------------------------
constexpr int CMS_FOLD_SEGS = 16;     // bin segments of k_cms_steady_add (HULK_STEADY_SEGS: 4 / 8 / 16 were swept, profiles/steady_fold.md)
constexpr int CMS_FOLD_PART = 1024;   // most counters of a row one workgroup keeps in LDS (8 KB of the 10,240 B six k_minimizer_fast workgroups leave)
inline int cms_fold_seg_bins(int32_t num_bins, int segs) { return (((num_bins + segs - 1) / segs) + 255) & ~255; }

__global__ __launch_bounds__(256) void k_cms_steady_sums(uint32_t *__restrict__ hists, unsigned long long *__restrict__ hsum,
                                                         const DevState *st, FlushBatch fb) {
    const uint32_t gomask = batch_gomask(st, fb);
    if (!st->skip_exact[fb.parity]) return;                      // (k_cms_steady_add raises the error)
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t B = (size_t)fb.num_bins;
    if (b >= (int64_t)B) return;
    // one bin per thread and spectrum: a wave's 64 dwords are contiguous whatever the base of the spectrum (an odd num_bins
    // leaves three ring slots of four off a 16-byte boundary, so nothing wider is loaded); every load is issued before the
    // first is used
    uint32_t v[RING_MAX];
    uint32_t slot = fb.ring_base % fb.ring_n;
#pragma unroll
    for (int t = 0; t < RING_MAX; t++) {
        v[t] = 0;
        if (t < (int)fb.count && ((gomask >> t) & 1u)) v[t] = hists[(size_t)slot * B + (size_t)b];
        if (++slot == fb.ring_n) slot = 0;
    }
    unsigned long long sum = 0;
#pragma unroll
    for (int t = 0; t < RING_MAX; t++) sum += v[t];
    hsum[b] = sum;
    slot = fb.ring_base % fb.ring_n;
#pragma unroll
    for (int t = 0; t < RING_MAX; t++) {
        if (t < (int)fb.count && ((gomask >> t) & 1u)) hists[(size_t)slot * B + (size_t)b] = 0;      // Wipe (kmerspectrum.go:58-64)
        if (++slot == fb.ring_n) slot = 0;
    }
}

// the books of a steady flush (one thread): the proof, the element count over the spectra that go, the 1 % rule
__device__ __forceinline__ void steady_books(DevState *st, const FlushBatch &fb, uint32_t gomask, bool proven) {
    if (!proven) { set_error(st, -34); return; }                                     // HULK_ERR_STATE: the host's verdict does not hold
    unsigned long long elems = 0; bool few = false;
    for (int t = 0; t < (int)fb.count; t++) {
        const unsigned used = st->used[fb.parity][ring_slot(fb, t)];
        if ((gomask >> t) & 1u) elems += used;
        else if (used != 0) few = true;                                              // "not used yet" (kmerspectrum.go:94-96)
    }
    if (few) set_error(st, -5);
    if (elems) atomicAdd(&st->n_elements, elems);
}

// grid (segments, depth, parts of a row); dynamic LDS: part_w 64-bit counters
__global__ __launch_bounds__(256) void k_cms_steady_add(const unsigned long long *__restrict__ hsum,
                                                        const uint16_t *__restrict__ pos16,
                                                        unsigned long long *__restrict__ ctr, int width, int part_w,
                                                        int seg_bins, DevState *st, FlushBatch fb) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long *lctr = (unsigned long long *)smem;       // [part_w]
    const uint32_t gomask = batch_gomask(st, fb);
    const bool proven = st->skip_exact[fb.parity] != 0u;
    const int tid = threadIdx.x, seg = blockIdx.x, d = blockIdx.y;
    if (tid == 0 && seg == 0 && d == 0 && blockIdx.z == 0) steady_books(st, fb, gomask, proven);
    if (!proven) return;
    const int p0 = (int)blockIdx.z * part_w;
    const int pw = width - p0 < part_w ? width - p0 : part_w;    // counters [p0, p0 + pw) of row d
    for (int i = tid; i < pw; i += 256) lctr[i] = 0;
    __syncthreads();
    const int64_t B = fb.num_bins;
    const int64_t b0 = (int64_t)seg * seg_bins, b1 = b0 + seg_bins < B ? b0 + seg_bins : B;
    const uint16_t *pd = pos16 + (size_t)d * (size_t)B;
    for (int64_t c0 = b0; c0 < b1; c0 += 8 * 256) {              // 8 x 256 bins of loads in flight
        unsigned long long h[8]; uint32_t p[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int64_t b = c0 + u * 256 + tid;
            const bool ok = b < b1;
            h[u] = ok ? hsum[b] : 0ull; p[u] = ok ? pd[b] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t q = p[u] - (uint32_t)p0;
            if (h[u] && q < (uint32_t)pw) atomicAdd(&lctr[q], h[u]);
        }
    }
    __syncthreads();
    for (int i = tid; i < pw; i += 256) {
        const unsigned long long s = lctr[i];
        if (s) atomicAdd(&ctr[(size_t)d * width + p0 + i], s);
    }
}

// HULK_STEADY_SEGSUM: k_cms_segsum + the wipe of the workgroup's own segment ...
__global__ __launch_bounds__(512) void k_cms_steady_segsum(uint32_t *__restrict__ hists, const uint16_t *__restrict__ pos16,
                                                           uint32_t *__restrict__ segsum, int depth, int width,
                                                           int seg_chunks, const DevState *st, FlushBatch fb) {
    cms_segsum<true>(hists, pos16, segsum, depth, width, seg_chunks, st, fb);
}
// ... and thread per counter, ctr += the sums of the intervals that go
__global__ __launch_bounds__(256) void k_cms_steady_segadd(const uint32_t *__restrict__ segsum,
                                                           unsigned long long *__restrict__ ctr, int depth, int width,
                                                           DevState *st, FlushBatch fb) {
    const uint32_t gomask = batch_gomask(st, fb);
    const bool proven = st->skip_exact[fb.parity] != 0u;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) steady_books(st, fb, gomask, proven);
    if (!proven || i >= depth * width) return;
    const int d = i / width, p = i - d * width;
    unsigned long long sum = 0;
    for (int t = 0; t < (int)fb.count; t++) {
        if (!((gomask >> t) & 1u)) continue;
        uint32_t sv[CMS_SEGS];
        const size_t at0 = (((size_t)t * depth + d) * CMS_SEGS) * width + p;
#pragma unroll
        for (int seg = 0; seg < CMS_SEGS; seg++) sv[seg] = segsum[at0 + (size_t)seg * width];   // independent loads
#pragma unroll
        for (int seg = 0; seg < CMS_SEGS; seg++) sum += sv[seg];
    }
    if (sum) ctr[i] += sum;
}

// base[t][d][seg][p] = counter (d,p) in front of segment seg of spectrum t; advances the persistent counters
__global__ __launch_bounds__(256) void k_cms_base(const uint32_t *__restrict__ segsum,
                                                  unsigned long long *__restrict__ ctr,
                                                  unsigned long long *__restrict__ base, int depth, int width,
                                                  const DevState *st, FlushBatch fb) {
    const uint32_t gomask = batch_gomask(st, fb);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= depth * width) return;
    const int d = i / width, p = i - d * width;
    unsigned long long run = ctr[i];
    for (int t = 0; t < (int)fb.count; t++) {
        if (!((gomask >> t) & 1u)) continue;
        uint32_t sv[CMS_SEGS];
        const size_t at0 = (((size_t)t * depth + d) * CMS_SEGS) * width + p;
#pragma unroll
        for (int seg = 0; seg < CMS_SEGS; seg++) sv[seg] = segsum[at0 + (size_t)seg * width];   // independent loads
#pragma unroll
        for (int seg = 0; seg < CMS_SEGS; seg++) { base[at0 + (size_t)seg * width] = run; run += sv[seg]; }
    }
    ctr[i] = run;
}

// Wave priority of the issue arbiter (0..3).  The count-min replay kernels with decay are chains of dependent LDS round trips, one
// workgroup per CU; beside them run kernels that fill the SIMDs' issue slots (k_minimizer_fast, k_jump_bin).  A replay wave that is
// ready should not queue behind eight of theirs.
__device__ __forceinline__ void set_wave_prio(int p) {
    if (p == 1) __builtin_amdgcn_s_setprio(1);
    else if (p == 2) __builtin_amdgcn_s_setprio(2);
    else if (p >= 3) __builtin_amdgcn_s_setprio(3);
}
// ------------------------------------------------------------------------------------------
// K3 with uniform scaling (0 < decay < 1), bin-order form.  Counter (d,p) right after stream element j
// is C(j) = w*C(j-1) + (v_j if element j hits it).  Over a bin segment holding elements [e0,e1):
//     C(e1-1) = w^(e1-e0) * C(e0-1) + sum{ v_j * w^(e1-1-j) : hits }
//   k_cmsd_segsum : the sum (one w^x per element; wave d owns row d: ascending bin order, reproducible) and the factor per segment
//   k_cmsd_base   : C in front of every (spectrum, segment), advancing the persistent fp64 counters
//   k_cmsd_freq   : replay in bin order with LDS counters normalised to a moving base element; zero bins are
//                   transparent; same-counter lanes of a 64-bin chunk resolve in lane order
// (fp64 sums are re-associated w.r.t. the reference's step-by-step scaling: ~1e-13 relative)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_cmsd_segsum(const uint32_t *__restrict__ hists, const uint16_t *__restrict__ pos16,
                                                     const uint32_t *__restrict__ eidx, const uint32_t *__restrict__ etot,
                                                     double *__restrict__ segadd, double *__restrict__ segfac,
                                                     uint32_t *__restrict__ sege0, int depth, int width, int seg_chunks,
                                                     double omega, const DevState *st, FlushBatch fb) {
    extern __shared__ __align__(16) unsigned char smem[];
    double *ladd = (double *)smem;                                // [depth][width]
    set_wave_prio(fb.prio);
    const int seg = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const uint32_t gomask = batch_gomask(st, fb);
    if (!((gomask >> t) & 1u)) return;
    for (int i = tid; i < depth * width; i += blockDim.x) ladd[i] = 0.0;
    __syncthreads();
    const size_t B = (size_t)fb.num_bins;
    const uint32_t *hist = hists + (size_t)ring_slot(fb, t) * B;
    const uint32_t *ei = eidx + (size_t)t * B;
    const int64_t b0 = (int64_t)seg * seg_chunks * 64, b1 = b0 + (int64_t)seg_chunks * 64;
    const uint32_t e0 = b0 < (int64_t)B ? ei[b0] : etot[t];
    const uint32_t e1 = b1 < (int64_t)B ? ei[b1] : etot[t];
    const double lnw = log(omega);                                // w^x = exp(x ln w): |x ln w| * 2^-53 relative, far below the tolerance
    if (tid == 0) { segfac[(size_t)t * CMS_SEGS + seg] = exp((double)(e1 - e0) * lnw); sege0[(size_t)t * CMS_SEGS + seg] = e0; }
    // Deterministic sums (round 3; before, every thread added its bins' terms to all rows with fp64 LDS atomics, in an order
    // that depended on the timing of the 8 waves: weights reproducible to ~1e-13, not to the bit).  Now the terms of a group of
    // 512 bins are computed once, one per thread, into an LDS staging array, and row d's counters are touched by wave d ONLY:
    // it walks the group's 8 chunks in order and adds lane l's term to its counter with one LDS atomic per chunk — same-address
    // lanes of one instruction resolve in the hardware's fixed lane order, successive instructions of a wave in program order,
    // so every counter receives its terms in ascending bin order, the same in every run.  Zero bins are transparent.
    double *stage = ladd + (size_t)depth * width;                 // [2][512]
    const int d = tid >> 6, lane = tid & 63;
    const uint16_t *pd = pos16 + (size_t)(d < depth ? d : 0) * B;
    const int64_t bend = b1 < (int64_t)B ? b1 : (int64_t)B;
    const int ngroups = (int)((bend - b0 + 511) / 512);
    // software pipeline: the terms of group g+1 are computed (VALU: one exp per thread) behind the LDS atomics of group g
    // (issued first, fire and forget), one barrier per group
    auto term = [&](uint32_t h, uint32_t e) { return h ? (double)h * exp((double)(e1 - 1u - e) * lnw) : 0.0; };
    uint32_t nh = 0, ne = 0;
    { const int64_t b = b0 + tid; if (b < bend) { nh = hist[b]; ne = ei[b]; } }
    if (ngroups > 0) stage[tid] = term(nh, ne);
    { const int64_t b = b0 + 512 + tid; nh = 0; ne = 0; if (b < bend) { nh = hist[b]; ne = ei[b]; } }
    uint16_t pn[8];
    auto fetch_pos = [&](int g) {
#pragma unroll
        for (int c = 0; c < 8; c++) { const int64_t b = b0 + (int64_t)g * 512 + c * 64 + lane; pn[c] = (d < depth && b < bend) ? pd[b] : (uint16_t)0; }
    };
    fetch_pos(0);
    __syncthreads();
    for (int g = 0; g < ngroups; g++) {
        uint16_t pp[8];
#pragma unroll
        for (int c = 0; c < 8; c++) pp[c] = pn[c];
        if (g + 1 < ngroups) fetch_pos(g + 1);
        if (d < depth) {
            const double *sg = stage + (g & 1) * 512;
            double wv[8];
#pragma unroll
            for (int c = 0; c < 8; c++) wv[c] = sg[c * 64 + lane];
#pragma unroll
            for (int c = 0; c < 8; c++) if (wv[c] != 0.0) atomicAdd(&ladd[d * width + pp[c]], wv[c]);
        }
        if (g + 1 < ngroups) {
            const uint32_t h = nh, e = ne;
            { const int64_t b = b0 + (int64_t)(g + 2) * 512 + tid; nh = 0; ne = 0; if (b < bend) { nh = hist[b]; ne = ei[b]; } }
            stage[((g + 1) & 1) * 512 + tid] = term(h, e);
        }
        __syncthreads();
    }
    __syncthreads();
    for (int i = tid; i < depth * width; i += blockDim.x) {
        const int dd = i / width, p = i - dd * width;
        segadd[((((size_t)t * depth) + dd) * CMS_SEGS + seg) * width + p] = ladd[i];
    }
}

__global__ __launch_bounds__(256) void k_cmsd_base(const double *__restrict__ segadd, const double *__restrict__ segfac,
                                                   double *__restrict__ ctrd, double *__restrict__ cstart, int depth,
                                                   int width, const DevState *st, FlushBatch fb) {
    const uint32_t gomask = batch_gomask(st, fb);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= depth * width) return;
    const int d = i / width, p = i - d * width;
    double C = ctrd[i];
    for (int t = 0; t < (int)fb.count; t++) {
        if (!((gomask >> t) & 1u)) continue;
        double sv[CMS_SEGS], fv[CMS_SEGS];
        const size_t at0 = (((size_t)t * depth + d) * CMS_SEGS) * width + p;
#pragma unroll
        for (int seg = 0; seg < CMS_SEGS; seg++) { sv[seg] = segadd[at0 + (size_t)seg * width]; fv[seg] = segfac[(size_t)t * CMS_SEGS + seg]; }
#pragma unroll
        for (int seg = 0; seg < CMS_SEGS; seg++) { cstart[at0 + (size_t)seg * width] = C; C = C * fv[seg] + sv[seg]; }
    }
    ctrd[i] = C;
}

// ------------------------------------------------------------------------------------------
// The replay: k_cms_freq, k_cms_freq_chain, k_cmsd_freq, k_cmsd_freq_chain are the four instances of cms_replay below.
// Workgroup (segment, spectrum): wave d < depth replays row d of the count-min sketch over the segment's bins in order, the
// [depth][width] counters in LDS.  The estimate of a bin is the minimum over the rows, which the row waves form with ONE 64-bit
// LDS atomic minimum per (row, bin) on a small staging array (integers, or non-negative doubles, whose bit patterns order
// like unsigned integers).  A barrier covers CMS_FG chunks of 64 bins; the combiner wave (d == depth) is one group behind:
// it reads one value per bin, writes f (fp64) and 1/f (fp32), wipes the spectrum and resets the staging slot.  No est arrays.
// The row waves are a chain of dependent LDS round trips, one workgroup per CU (112 KB of counters), so the number of round
// trips per chunk IS the kernel's time; the per-bin inputs of the WHOLE next group are requested before the current group is
// computed: nothing else hides their latency.
//
// Arithmetic (CmsInt / CmsDecay) owns the counter type, where the counters start, the bit pattern of "no value", the row
// step of either order and the combiner's conversion.
// Order: LDS — the LDS keeps the bin order by itself: a returning atomic add (ds_add_rtn_u64 / ds_add_rtn_f64) hands back the
// counter as it stood before this lane's add, same-address lanes of one instruction are applied in ascending lane order, a
// wave's instructions in program order (tools/ubench/lds_atomic_order.hip; lds_order_verified below).  Chain — the FALLBACK
// for a device whose LDS does not (HULK_FLAG_CMS_CHAIN forces it): the order inside a 64-bin chunk comes from the static table
// k_build_chains wrote — meta8 = {the nearest LOWER lane of the chunk on the same counter (64: none), bit 7: the last lane on
// its counter} — followed with ballots and register exchanges (chain_resolve); the LDS is only read by the first lane of a
// counter's run and written by its last.  The same additions in the same order: bit-identical to the LDS order (tested), at
// 1.3x (integer) and 1.5x (decay) its time (profiles/cms_replay.txt; docs/EXPERIMENTS.md has both forms' history).
// ------------------------------------------------------------------------------------------
constexpr int CMS_FG = 8;             // chunks of 64 bins per barrier group
constexpr int CMS_GB = CMS_FG * 64;
constexpr int CMSD_WAVE_PRIO = 0;     // s_setprio of the replay kernels (set_wave_prio)

// Chain order, one chunk of one row: a lane is computed once its predecessor on the same counter is (whether it is comes from
// the wave's ballot of finished lanes).  add(before) returns the counter after this lane's bin, given the counter before it
// — what the returning atomic hands back in the LDS order — and posts the lane's estimate.
template <class T, class Add>
__device__ __forceinline__ void chain_resolve(T *rc, uint32_t p, uint32_t m, bool live, Add add) {
    const uint32_t prev = m & 0x7fu;
    bool ready = false; T Sn = 0;
    if (prev >= 64u) { Sn = add(rc[p]); ready = true; }              // first lane of the chunk on this counter: LDS state
    unsigned long long done = __ballot(ready);
    while (done != ~0ull) {
        const T before = __shfl(Sn, (int)(prev & 63u));
        const bool pr = (done >> (prev & 63u)) & 1ull;
        if (!ready && pr) { Sn = add(before); ready = true; }
        done = __ballot(ready);
    }
    if ((m & 0x80u) && live) rc[p] = Sn;
}

// Integer counters (decay_ratio == 1): est = counter before + own count is the reference's counter after Add (countmin.go:122-127).
struct CmsInt {
    using Ctr = unsigned long long;
    static constexpr unsigned long long NONE = ~0ull;
    static constexpr bool BY_SPECTRUM = true;    // "bin not in the stream" is a zero of the spectrum: the combiner needs its values and wipes only the others
    static constexpr bool PRUNES = true;         // k_flush_decide's skip_exact leaves only the wipe to do
    static constexpr bool REBASES = false;
    const Ctr *__restrict__ start;               // k_cms_base: the counters in front of every (spectrum, segment)
    __device__ void prepare(int, int, int, size_t) {}
    __device__ uint32_t elem(int64_t) const { return 0u; }
    __device__ void rebase(Ctr *, uint32_t, int, int) {}
    __device__ void lds_step(Ctr *rc, unsigned long long *est, uint32_t h, uint32_t p, uint32_t) const {
        if (h) atomicMin(est, atomicAdd(&rc[p], (Ctr)h) + h);
    }
    __device__ void chain_step(Ctr *rc, unsigned long long *est, uint32_t h, uint32_t p, uint32_t, uint32_t m, bool live) const {
        chain_resolve(rc, p, m, live, [=](Ctr before) { const Ctr Sn = before + h; if (h) atomicMin(est, Sn); return Sn; });
    }
    static __device__ double value(unsigned long long bits) { return (double)bits; }
};

// fp64 counters with uniform scaling (0 < decay < 1).  A counter is kept ADDITIVELY normalised to a base element index,
// S = sum over its elements i of v_i * w^-(i - base), so that its value right after element j is S * w^(j - base): an element
// only ADDS g = v * w^-(j - base) to its counter.  Every `period` elements the base moves on and the row's counters are
// rescaled by w^period (the period keeps w^-(j - base) far below the fp64 range for any decay < 1).  Zero bins are transparent;
// +inf is "bin not in the stream".  (Rounding: C = (S + v*wi) * wf — a re-association of the reference's step-by-step
// scaling, ~1e-13 relative; bit-reproducible from run to run.)
__shared__ double cmsd_tabf_lo[64], cmsd_tabf_hi[66], cmsd_tabi_lo[64], cmsd_tabi_hi[66];   // w^x and w^-x for x = lo + 64 hi
struct CmsDecay {
    using Ctr = double;
    static constexpr unsigned long long NONE = 0x7FF0000000000000ull;
    static constexpr bool BY_SPECTRUM = false;   // the combiner sees +inf and wipes every bin
    static constexpr bool PRUNES = false;
    static constexpr bool REBASES = true;        // rebase() has work to do at a chunk whatever its bins hold
    const double *__restrict__ start;            // k_cmsd_base's cstart: the value right after element e0 - 1, S at base = e0 - 1
    const uint32_t *__restrict__ eidx, *__restrict__ sege0;
    double omega;
    const uint32_t *ei; long long base; int period; double wperiod;
    __device__ void prepare(int t, int seg, int tid, size_t B) {
        const double lnw = log(omega);                               // < 0
        // elements per base: |ln w| * (period + 64) <= 600  =>  w^-(j - base) <= e^600 (counters stay below ~1e270)
        period = 4032;
        if (-lnw * (double)(period + 64) > 600.0) period = (int)(600.0 / -lnw) - 64;
        period &= ~63;
        if (period < 64) period = 64;
        wperiod = exp((double)period * lnw);
        if (tid < 64) { cmsd_tabf_lo[tid] = exp((double)tid * lnw); cmsd_tabi_lo[tid] = exp(-(double)tid * lnw); }
        if (tid >= 64 && tid < 64 + 66) { const int x = tid - 64; cmsd_tabf_hi[x] = exp((double)(64 * x) * lnw); cmsd_tabi_hi[x] = exp(-(double)(64 * x) * lnw); }
        ei = eidx + (size_t)t * B;
        base = (long long)sege0[(size_t)t * CMS_SEGS + seg] - 1;
    }
    __device__ uint32_t elem(int64_t b) const { return ei[b]; }
    // move the base on when the chunk's elements would leave the tables (wave-uniform: element indices ascend with the lane;
    // lane 0 holds the chunk's first)
    __device__ void rebase(Ctr *rv, uint32_t j, int lane, int width) {
        const long long jfirst = (long long)__builtin_amdgcn_readfirstlane((int)j);
        while (jfirst - base > (long long)period) {
            for (int i = lane; i < width; i += 64) rv[i] *= wperiod;
            base += period;
        }
    }
    // ~15 VALU + 6 LDS instructions per (row, chunk), the eight atomics of a group in flight together
    __device__ void lds_step(Ctr *rv, unsigned long long *est, uint32_t h, uint32_t p, uint32_t j) const {
        if (h) {
            const uint32_t x = (uint32_t)((long long)j - base);          // 1 .. period + 64
            const double wi = cmsd_tabi_lo[x & 63u] * cmsd_tabi_hi[x >> 6], wf = cmsd_tabf_lo[x & 63u] * cmsd_tabf_hi[x >> 6];
            const double gv = (double)h * wi;
            const double before = atomicAdd(&rv[p], gv);                 // ds_add_rtn_f64: the counter in bin order
            atomicMin(est, (unsigned long long)__double_as_longlong((before + gv) * wf));
        }
    }
    __device__ void chain_step(Ctr *rv, unsigned long long *est, uint32_t h, uint32_t p, uint32_t j, uint32_t m, bool live) const {
        const uint32_t x = h ? (uint32_t)((long long)j - base) : 0u;     // 1 .. period + 64 (unused for bins not in the stream)
        const double wi = cmsd_tabi_lo[x & 63u] * cmsd_tabi_hi[x >> 6], wf = cmsd_tabf_lo[x & 63u] * cmsd_tabf_hi[x >> 6];
        const double gv = (double)h * wi;
        chain_resolve(rv, p, m, live, [=](double before) {
            if (!h) return before;
            const double Sn = before + gv;
            atomicMin(est, (unsigned long long)__double_as_longlong(Sn * wf));
            return Sn;
        });
    }
    static __device__ double value(unsigned long long bits) { return __longlong_as_double((long long)bits); }
};

template <bool CHAIN, class A>
__device__ __forceinline__ void cms_replay(A ar, uint32_t *__restrict__ hists, const uint16_t *__restrict__ pos16,
                                           const uint8_t *__restrict__ meta8, double *__restrict__ f64, float *__restrict__ rcp32,
                                           int depth, int width, int seg_chunks, size_t row_stride, DevState *st,
                                           const FlushBatch &fb) {
    using Ctr = typename A::Ctr;
    extern __shared__ __align__(16) unsigned char smem[];
    Ctr *lctr = (Ctr *)smem;                                                     // [depth][width]
    unsigned long long *smin = (unsigned long long *)(lctr + (size_t)depth * width);   // [2][CMS_GB] minimum over the rows, as bits
    const int seg = blockIdx.x, t = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, d = tid >> 6;                  // waves 0..depth-1: rows; wave depth: combiner
    const uint32_t gomask = batch_gomask(st, fb);
    const bool go = (gomask >> t) & 1u;
    const uint32_t slot = ring_slot(fb, t);
    if (seg == 0 && tid == 0) {
        const unsigned used = st->used[fb.parity][slot];
        if (used != 0 && !go) set_error(st, -5);                                 // "not used yet" (kmerspectrum.go:94-96)
        if (go) atomicAdd(&st->n_elements, (unsigned long long)used);
    }
    if (!go) return;
    const size_t B = (size_t)fb.num_bins;
    uint32_t *hist = hists + (size_t)slot * B;
    const int64_t b0 = (int64_t)seg * seg_chunks * 64;
    if (A::PRUNES && st->skip_exact[fb.parity]) {                                // k_flush_decide: only Wipe is left to do
        const int64_t w1 = b0 + (int64_t)seg_chunks * 64;
        for (int64_t b = b0 + tid; b < w1 && b < (int64_t)B; b += blockDim.x) hist[b] = 0;
        return;
    }
    ar.prepare(t, seg, tid, B);
    {
        const Ctr *bt = ar.start + (((size_t)t * depth) * CMS_SEGS) * width;
        for (int i = tid; i < depth * width; i += blockDim.x) {
            const int dd = i / width, p = i - dd * width;
            lctr[i] = bt[((size_t)dd * CMS_SEGS + seg) * width + p];
        }
        for (int i = tid; i < 2 * CMS_GB; i += blockDim.x) smin[i] = A::NONE;
    }
    __syncthreads();
    double *ft = f64 + (size_t)t * B;
    float *rt = rcp32 + (size_t)t * row_stride;
    const int ngroups = (seg_chunks + CMS_FG - 1) / CMS_FG;
    const uint16_t *pd = pos16 + (size_t)(d < depth ? d : 0) * B;
    const uint8_t *md = CHAIN ? meta8 + (size_t)(d < depth ? d : 0) * B : nullptr;
    Ctr *rc = lctr + (size_t)(d < depth ? d : 0) * width;
    struct Group { uint32_t h[CMS_FG], p[CMS_FG], j[CMS_FG], m[CMS_FG]; } nx, cu;   // spectrum value, counter, element index, meta8
    auto fetch = [&](int g) {
#pragma unroll
        for (int c = 0; c < CMS_FG; c++) {
            const int ch = g * CMS_FG + c;
            const int64_t b = b0 + (int64_t)ch * 64 + lane;
            nx.h[c] = 0; nx.p[c] = 0; nx.j[c] = 0; nx.m[c] = 64u | 0x80u;
            if ((d < depth || A::BY_SPECTRUM) && ch < seg_chunks && b < (int64_t)B) {
                nx.h[c] = hist[b];
                if (d < depth) { nx.p[c] = pd[b]; nx.j[c] = ar.elem(b); if (CHAIN) nx.m[c] = md[b]; }
            }
        }
    };
    fetch(0);
    uint32_t ph[CMS_FG];                                        // combiner: spectrum values of the group it finishes next
#pragma unroll
    for (int c = 0; c < CMS_FG; c++) ph[c] = 0;
    for (int g = 0; g <= ngroups; g++) {
        cu = nx;
        if (g + 1 < ngroups) fetch(g + 1);
        if (d < depth && g < ngroups) {
            unsigned long long *my = smin + (size_t)(g & 1) * CMS_GB + lane;
#pragma unroll
            for (int c = 0; c < CMS_FG; c++) {
                const int ch = g * CMS_FG + c;
                // a chunk beyond the segment's end holds no bin.  k_cms_freq is left without this test: its step does nothing
                // where h == 0, and with the test (eight more scalar compares and exec masks per group) it took 57.61 us
                // against the parent's 57.29, spread 0.09; without it 55.70 against 56.92 (profiles/cms_replay.txt)
                if ((CHAIN || A::REBASES) && ch >= seg_chunks) continue;
                ar.rebase(rc, cu.j[c], lane, width);
                if (CHAIN) ar.chain_step(rc, &my[c * 64], cu.h[c], cu.p[c], cu.j[c], cu.m[c], b0 + (int64_t)ch * 64 + lane < (int64_t)B);
                else ar.lds_step(rc, &my[c * 64], cu.h[c], cu.p[c], cu.j[c]);
            }
        }
        if (d == depth && g > 0) {
            unsigned long long *src = smin + (size_t)((g - 1) & 1) * CMS_GB + lane;
#pragma unroll
            for (int c = 0; c < CMS_FG; c++) {
                const int ch = (g - 1) * CMS_FG + c;
                const int64_t b = b0 + (int64_t)ch * 64 + lane;
                if (ch < seg_chunks && b < (int64_t)B) {
                    const bool look = !A::BY_SPECTRUM || ph[c] != 0;
                    unsigned long long bits = A::NONE;
                    if (look) { bits = src[c * 64]; src[c * 64] = A::NONE; }
                    if (A::BY_SPECTRUM ? look : bits != A::NONE) {
                        const double f = A::value(bits);
                        ft[b] = f; rt[b] = (float)(1.0 / f);
                    } else { ft[b] = 0.0; rt[b] = __builtin_nanf(""); }
                    if (look) hist[b] = 0;                           // Wipe (kmerspectrum.go:58-64)
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CMS_FG; c++) ph[c] = cu.h[c];       // group g is finished by the combiner at g+1
        __syncthreads();
    }
}

#define CMS_REPLAY_IO uint32_t *__restrict__ hists, const uint16_t *__restrict__ pos16, double *__restrict__ f64, \
                      float *__restrict__ rcp32, int depth, int width, int seg_chunks, size_t row_stride, DevState *st, FlushBatch fb
__global__ __launch_bounds__(512) void k_cms_freq(const unsigned long long *__restrict__ base, CMS_REPLAY_IO) {
    cms_replay<false>(CmsInt{base}, hists, pos16, nullptr, f64, rcp32, depth, width, seg_chunks, row_stride, st, fb);
}
__global__ __launch_bounds__(512) void k_cms_freq_chain(const unsigned long long *__restrict__ base, const uint8_t *__restrict__ meta8,
                                                        CMS_REPLAY_IO) {
    cms_replay<true>(CmsInt{base}, hists, pos16, meta8, f64, rcp32, depth, width, seg_chunks, row_stride, st, fb);
}
__global__ __launch_bounds__(512) void k_cmsd_freq(const double *__restrict__ cstart, const uint32_t *__restrict__ eidx,
                                                   const uint32_t *__restrict__ sege0, double omega, CMS_REPLAY_IO) {
    set_wave_prio(fb.prio);
    cms_replay<false>(CmsDecay{cstart, eidx, sege0, omega}, hists, pos16, nullptr, f64, rcp32, depth, width, seg_chunks, row_stride, st, fb);
}
__global__ __launch_bounds__(512) void k_cmsd_freq_chain(const double *__restrict__ cstart, const uint32_t *__restrict__ eidx,
                                                         const uint32_t *__restrict__ sege0, double omega,
                                                         const uint8_t *__restrict__ meta8, CMS_REPLAY_IO) {
    cms_replay<true>(CmsDecay{cstart, eidx, sege0, omega}, hists, pos16, meta8, f64, rcp32, depth, width, seg_chunks, row_stride, st, fb);
}
#undef CMS_REPLAY_IO

// ==========================================================================================
// Concept drift (decay_ratio != 1): reference src/countmin/countmin.go:49-56,103-110,141-147 and
// src/histosketch/histosketch.go:79-81,139-153.
//
// Count-min with uniform scaling (0 < decay < 1): every Add() first multiplies ALL counters by
// w = exp(-decay).  With i = index of an element inside its flush (ascending non-zero bins), the
// counter (d,g) right after element i is  C0*w^(i+1) + sum{ v_j * w^(i-j) : j <= i, pos_d(b_j)=g },
// i.e. along a chain the first-order recurrence  S_m = w^(gap_m) * S_{m-1} + v_m  — an affine scan.
// (The reference multiplies step by step; the closed form differs by accumulated rounding of
// ~gap*2^-53 relative, far inside the 1e-5 tolerance the north star states for CWS values.)
// ==========================================================================================

// element index of every bin = number of non-zero bins in front of it.  grid = (blocks, count)
constexpr int EIDX_BLOCK = 2048;
__global__ __launch_bounds__(256) void k_elem_count(const uint32_t *__restrict__ hists,
                                                    uint32_t *__restrict__ blkcnt, int nblk, FlushBatch fb) {
    __shared__ unsigned red[4];
    const int t = blockIdx.y, blk = blockIdx.x;
    const uint32_t *hist = hists + (size_t)ring_slot(fb, t) * (size_t)fb.num_bins;
    unsigned cnt = 0;
    for (int x = 0; x < EIDX_BLOCK / 256; x++) {
        const int32_t b = blk * EIDX_BLOCK + x * 256 + threadIdx.x;
        if (b < fb.num_bins) cnt += hist[b] != 0;
    }
    for (int off = 32; off; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane_id() == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) blkcnt[(size_t)t * nblk + blk] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void k_elem_index(const uint32_t *__restrict__ hists,
                                                    const uint32_t *__restrict__ blkcnt,
                                                    uint32_t *__restrict__ eidx, uint32_t *__restrict__ etot,
                                                    int nblk, FlushBatch fb, DevState *st) {
    __shared__ unsigned red[4];
    __shared__ unsigned wsum[4];
    const int t = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const size_t B = (size_t)fb.num_bins;
    const uint32_t *hist = hists + (size_t)ring_slot(fb, t) * B;
    // offset of this block = sum of the counts of the blocks in front of it
    unsigned off = 0, all = 0;
    for (int x = tid; x < nblk; x += 256) { const unsigned c = blkcnt[(size_t)t * nblk + x]; all += c; if (x < blk) off += c; }
    for (int o = 32; o; o >>= 1) { off += __shfl_xor(off, o); all += __shfl_xor(all, o); }
    if (lane == 0) { red[wid] = off; wsum[wid] = all; }
    __syncthreads();
    off = red[0] + red[1] + red[2] + red[3];
    if (blk == 0 && tid == 0) {
        const unsigned total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        etot[t] = total;
        // the number of elements IS KmerSpectrum.Cardinality() (kmerspectrum.go:53-55): with decay the flush takes the 1 %
        // rule's count from here instead of a k_count_used pass of its own (26 us per 16 spectra at k = 31)
        st->used[fb.parity][ring_slot(fb, t)] = total;
    }
    __syncthreads();
    // 8 consecutive bins per thread
    const int32_t b0 = blk * EIDX_BLOCK + tid * 8;
    unsigned nz[8]; unsigned mine = 0;
#pragma unroll
    for (int x = 0; x < 8; x++) { nz[x] = (b0 + x < fb.num_bins) ? (hist[b0 + x] != 0) : 0u; mine += nz[x]; }
    unsigned incl = wave_scan_incl(mine);
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    unsigned before = off + incl - mine;
    for (int x = 0; x < wid; x++) before += wsum[x];
#pragma unroll
    for (int x = 0; x < 8; x++) { if (b0 + x < fb.num_bins) eidx[(size_t)t * B + b0 + x] = before; before += nz[x]; }
}

}  // namespace

// ---------------------------------------------------------------------------- host wrappers
hipError_t launch_count_used(hipStream_t s, const uint32_t *d_hists, DevState *st, const FlushBatch &fb) {
    int blocks = (fb.num_bins + 2047) / 2048; if (blocks > 128) blocks = 128;
    prof_mark(s, "k_count_used");
    hipLaunchKernelGGL(k_count_used, dim3(blocks, fb.count), dim3(256), 0, s, d_hists, st, fb);
    return hipGetLastError();
}

hipError_t launch_cms_binorder(hipStream_t s, uint32_t *d_hists, const uint16_t *d_pos16, const uint8_t *d_meta8,
                               unsigned long long *d_ctr, uint32_t *d_segsum, unsigned long long *d_base,
                               double *d_f64, float *d_rcp32, int depth, int width, size_t row_stride,
                               DevState *st, const FlushBatch &fb, bool chain) {
    const int seg_chunks = cms_seg_chunks(fb.num_bins);
    const size_t lds1 = (size_t)depth * width * 4;
    const size_t lds3 = (size_t)depth * width * 8 + (size_t)2 * CMS_GB * 8;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void *)k_cms_freq, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_cms_freq_chain, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    prof_mark(s, "k_cms_segsum");
    hipLaunchKernelGGL(k_cms_segsum, dim3(CMS_SEGS, fb.count), dim3(512), lds1, s, d_hists, d_pos16, d_segsum, depth, width,
                       seg_chunks, st, fb);
    prof_mark(s, "k_cms_base");
    hipLaunchKernelGGL(k_cms_base, dim3((depth * width + 255) / 256), dim3(256), 0, s, d_segsum, d_ctr, d_base, depth, width, st, fb);
    if (chain) {
        prof_mark(s, "k_cms_freq_chain");
        hipLaunchKernelGGL(k_cms_freq_chain, dim3(CMS_SEGS, fb.count), dim3(512), lds3, s, d_base, d_meta8, d_hists, d_pos16, d_f64,
                           d_rcp32, depth, width, seg_chunks, row_stride, st, fb);
    }
    else {
        prof_mark(s, "k_cms_freq");
        hipLaunchKernelGGL(k_cms_freq, dim3(CMS_SEGS, fb.count), dim3(512), lds3, s, d_base, d_hists, d_pos16, d_f64,
                           d_rcp32, depth, width, seg_chunks, row_stride, st, fb);
    }
    return hipGetLastError();
}

hipError_t launch_cms_steady(hipStream_t s, uint32_t *d_hists, const uint16_t *d_pos16, unsigned long long *d_ctr,
                             uint32_t *d_segsum, unsigned long long *d_hsum, int depth, int width, DevState *st,
                             const FlushBatch &fb) {
    static const bool segsum_form = HULK_EXP_ENV("HULK_STEADY_SEGSUM") != nullptr;
    if (segsum_form) {
        prof_mark(s, "k_cms_steady_sums");
        hipLaunchKernelGGL(k_cms_steady_segsum, dim3(CMS_SEGS, fb.count), dim3(512), (size_t)depth * width * 4, s, d_hists, d_pos16,
                           d_segsum, depth, width, cms_seg_chunks(fb.num_bins), st, fb);
        prof_mark(s, "k_cms_steady_add");
        hipLaunchKernelGGL(k_cms_steady_segadd, dim3((depth * width + 255) / 256), dim3(256), 0, s, d_segsum, d_ctr, depth, width, st, fb);
        return hipGetLastError();
    }
    if (!d_hsum || fb.num_bins <= 0 || width <= 0 || fb.count > (uint32_t)RING_MAX) return hipErrorInvalidValue;
    static const int segs = [] { const char *e = HULK_EXP_ENV("HULK_STEADY_SEGS"); const int v = e ? atoi(e) : CMS_FOLD_SEGS; return v < 1 ? 1 : v > 64 ? 64 : v; }();
    const int parts = (width + CMS_FOLD_PART - 1) / CMS_FOLD_PART, part_w = (width + parts - 1) / parts;
    prof_mark(s, "k_cms_steady_sums");
    hipLaunchKernelGGL(k_cms_steady_sums, dim3((fb.num_bins + 255) / 256), dim3(256), 0, s, d_hists, d_hsum, st, fb);
    prof_mark(s, "k_cms_steady_add");
    hipLaunchKernelGGL(k_cms_steady_add, dim3(segs, depth, parts), dim3(256), (size_t)part_w * 8, s, d_hsum, d_pos16, d_ctr, width,
                       part_w, cms_fold_seg_bins(fb.num_bins, segs), st, fb);
    return hipGetLastError();
}

size_t cms_binorder_entries(int depth, int width) { return (size_t)depth * CMS_SEGS * width; }

hipError_t launch_cmsd_binorder(hipStream_t s, uint32_t *d_hists, const uint16_t *d_pos16, const uint8_t *d_meta8,
                                const uint32_t *d_eidx, const uint32_t *d_etot, double *d_ctrd, double *d_segadd,
                                double *d_segfac, uint32_t *d_sege0, double *d_cstart, double *d_f64, float *d_rcp32,
                                int depth, int width, size_t row_stride, double omega, DevState *st, const FlushBatch &fb_in,
                                hipEvent_t freq_begin, hipEvent_t freq_end, bool chain_form) {
    FlushBatch fb = fb_in;
    const int seg_chunks = cms_seg_chunks(fb.num_bins);
    if (depth > 8) return hipErrorInvalidValue;                     // k_cmsd_segsum: one wave per row, 8 waves
    { static const char *e = HULK_EXP_ENV("HULK_CMSD_PRIO"); fb.prio = e ? atoi(e) : CMSD_WAVE_PRIO; }
    const size_t lds1 = (size_t)depth * width * 8 + (size_t)2 * 512 * 8;
    const size_t lds3 = (size_t)depth * width * 8 + (size_t)2 * CMS_GB * 8;
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void *)k_cmsd_segsum, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_cmsd_freq, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_cmsd_freq_chain, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    prof_mark(s, "k_cmsd_segsum");
    hipLaunchKernelGGL(k_cmsd_segsum, dim3(CMS_SEGS, fb.count), dim3(512), lds1, s, d_hists, d_pos16, d_eidx, d_etot, d_segadd,
                       d_segfac, d_sege0, depth, width, seg_chunks, omega, st, fb);
    prof_mark(s, "k_cmsd_base");
    hipLaunchKernelGGL(k_cmsd_base, dim3((depth * width + 255) / 256), dim3(256), 0, s, d_segadd, d_segfac, d_ctrd, d_cstart,
                       depth, width, st, fb);
    if (freq_begin) { const hipError_t e = hipEventRecord(freq_begin, s); if (e != hipSuccess) return e; }   // bench.py: k_cmsd_freq alone
    const bool chain = chain_form || HULK_EXP_ENV("HULK_CMSD_CHAIN") != nullptr;   // the fallback (lds_order_verified / HULK_FLAG_CMS_CHAIN)
    if (chain) {
        prof_mark(s, "k_cmsd_freq_chain");
        hipLaunchKernelGGL(k_cmsd_freq_chain, dim3(CMS_SEGS, fb.count), dim3(512), lds3, s, d_cstart, d_eidx, d_sege0, omega, d_meta8,
                           d_hists, d_pos16, d_f64, d_rcp32, depth, width, seg_chunks, row_stride, st, fb);
    }
    else {
        prof_mark(s, "k_cmsd_freq");
        hipLaunchKernelGGL(k_cmsd_freq, dim3(CMS_SEGS, fb.count), dim3(512), lds3, s, d_cstart, d_eidx, d_sege0, omega, d_hists,
                           d_pos16, d_f64, d_rcp32, depth, width, seg_chunks, row_stride, st, fb);
    }
    if (freq_end) { const hipError_t e = hipEventRecord(freq_end, s); if (e != hipSuccess) return e; }
    return hipGetLastError();
}

hipError_t launch_elem_index(hipStream_t s, const uint32_t *d_hists, uint32_t *d_blkcnt, uint32_t *d_eidx,
                             uint32_t *d_etot, const FlushBatch &fb, DevState *st) {
    const int nblk = (fb.num_bins + EIDX_BLOCK - 1) / EIDX_BLOCK;
    prof_mark(s, "k_elem_count");
    hipLaunchKernelGGL(k_elem_count, dim3(nblk, fb.count), dim3(256), 0, s, d_hists, d_blkcnt, nblk, fb);
    prof_mark(s, "k_elem_index");
    hipLaunchKernelGGL(k_elem_index, dim3(nblk, fb.count), dim3(256), 0, s, d_hists, d_blkcnt, d_eidx, d_etot, nblk, fb, st);
    return hipGetLastError();
}

int elem_index_blocks(int32_t num_bins) { return (num_bins + EIDX_BLOCK - 1) / EIDX_BLOCK; }

// ------------------------------------------------------------------------------------------
// The hardware property k_cms_freq / k_cmsd_freq / k_cmsd_segsum rest on, checked on the device itself once per process and
// device (hulk_create): for ONE returning LDS atomic add (ds_add_rtn_u64 / ds_add_rtn_f64) whose lanes hit the same address, the
// value a lane gets back is the value before the instruction plus the operands of the LOWER lanes on that address (ascending
// lane order), and the instructions of a wave are applied in program order.  Patterns: all 64 lanes on one address, pairs,
// pseudo-random partitions into 1..61 groups; two instructions back to back on different partitions.  Every lane checks its own
// returned value against the sum it can form from the wave's operands (readlane).  out[0] / out[1]: lanes out of order for
// u64 / f64.  (tools/ubench/lds_atomic_order.hip is the stand-alone form of the same test.)
// ------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(64) void k_lds_order_probe(unsigned int *out, int rounds, unsigned int sabotage) {
    __shared__ unsigned long long su[64];
    __shared__ double sd[64];
    const int l = threadIdx.x;
    unsigned bad_u = 0, bad_d = 0;
    uint32_t rng = 0x9E3779B9u * (uint32_t)(l + 1);
    for (int r = 0; r < rounds; r++) {
        const int mode = r & 3;
        rng = rng * 1664525u + 1013904223u; const uint32_t ra = rng >> 8;
        rng = rng * 1664525u + 1013904223u; const uint32_t rb = rng >> 8;
        // (range reduction by multiply-shift, not `ra % m`: for operands it can prove to be below 2^24 hipcc 7.2 expands the
        // remainder through v_rcp_iflag_f32 and never corrects an OVER-estimated quotient — x = q * m - 1 near 2^24 comes back as
        // 0xFFFFFF; the first version of this probe indexed the LDS with that and "found" 32 lanes out of order.
        // tools/ubench/urem24_check.hip, profiles/r06_urem24.txt.  No kernel of the library has such an operand pair.)
        const int p0 = mode == 0 ? 0 : mode == 1 ? l / 2 : (int)((ra * (uint32_t)(1 + r % 61)) >> 24);
        const int p1 = mode == 0 ? 0 : mode == 1 ? (63 - l) / 2 : (int)((rb * (uint32_t)(1 + r % 59)) >> 24);
        const unsigned long long v0 = 1ull + (unsigned)l, v1 = 1000ull + (unsigned)l;
        su[l] = 7ull * (unsigned)l; sd[l] = (double)(7 * l);
        __syncthreads();
        const unsigned long long a_u = atomicAdd(&su[p0], v0);
        const unsigned long long b_u = atomicAdd(&su[p1], v1);
        const double a_d = atomicAdd(&sd[p0], (double)v0);
        const double b_d = atomicAdd(&sd[p1], (double)v1);
        // expectation: start value + lower lanes of the same instruction (+ every lane of the earlier instruction) on that address
        unsigned long long ea = 7ull * (unsigned)p0, eb = 7ull * (unsigned)p1;
        for (int j = 0; j < 64; j++) {
            const int q0 = __builtin_amdgcn_readlane(p0, j), q1 = __builtin_amdgcn_readlane(p1, j);
            if (q0 == p0 && j < l) ea += 1ull + (unsigned)j;
            if (q0 == p1) eb += 1ull + (unsigned)j;
            if (q1 == p1 && j < l) eb += 1000ull + (unsigned)j;
        }
        if (sabotage) ea += (unsigned)(l == 5);                   // (self-test of the checker: HULK_LDS_PROBE_SABOTAGE, profiling build)
        bad_u += (a_u != ea) + (b_u != eb);
        bad_d += (a_d != (double)ea) + (b_d != (double)eb);       // (sums of small integers: exact in fp64)
        __syncthreads();
    }
    for (int off = 32; off; off >>= 1) { bad_u += __shfl_xor(bad_u, off); bad_d += __shfl_xor(bad_d, off); }
    if (l == 0) { out[0] = bad_u; out[1] = bad_d; }
}
}  // namespace

// 1: the LDS applies same-address lanes in ascending lane order (what every gfx950 measured so far does), 0: it does not — the
// count-min replay then runs k_cms_freq_chain / k_cmsd_freq_chain —, < 0: the probe could not run (hipError_t negated).
int lds_order_verified(int device) {
    static std::mutex mu;
    static int cache[64];
    static bool init = false;
    std::lock_guard<std::mutex> lk(mu);
    if (!init) { for (int &x : cache) x = -1000000; init = true; }
    if (device >= 0 && device < 64 && cache[device] != -1000000) return cache[device];
    unsigned int *d_out = nullptr, h[2] = {1, 1};
    hipError_t e = hipMalloc((void **)&d_out, 8);
    if (e == hipSuccess) {
        const unsigned sabotage = HULK_EXP_ENV("HULK_LDS_PROBE_SABOTAGE") != nullptr;
        hipLaunchKernelGGL(k_lds_order_probe, dim3(1), dim3(64), 0, 0, d_out, 488, sabotage);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(h, d_out, 8, hipMemcpyDeviceToHost);
        (void)hipFree(d_out);
    }
    const int res = e != hipSuccess ? -(int)e : (h[0] == 0 && h[1] == 0) ? 1 : 0;
    if (res == 0)
        fprintf(stderr, "libhulkhip: device %d: the LDS does not apply same-address lanes of a returning atomic in ascending lane order "
                        "(%u u64, %u f64 lanes out of order): the count-min replay uses the chain-form kernels\n", device, h[0], h[1]);
    if (device >= 0 && device < 64 && res >= 0) cache[device] = res;
    return res;
}

// Static chain tables of the bin-order count-min kernels (built once per context): for row d the counter position
// g = jump(bin + d*bin, width) of every bin (countmin.go:122-125), and per 64-bin chunk which earlier lane of the chunk
// hits the same counter (bits 0-6, 64 = none) and whether the bin is the last one of the chunk on its counter (bit 7).
// One wave per (row, chunk).  (A host loop did this until round 2: 7 * k^4 jump hashes, 70 ms of every hulk_create at k = 21.)
namespace {
__global__ __launch_bounds__(256) void k_build_chains(uint16_t *__restrict__ pos16, uint8_t *__restrict__ meta8, int32_t B, int width) {
    const int lane = lane_id();
    const int32_t chunk = (int32_t)blockIdx.x * 4 + (int32_t)(threadIdx.x >> 6);
    const int d = (int)blockIdx.y;
    const int32_t b = chunk * 64 + lane;
    if (chunk * 64 >= B) return;
    const bool valid = b < B;
    const uint32_t pos = valid ? (uint32_t)jump_hash((uint64_t)b + (uint64_t)d * (uint64_t)b, width) : 0xffffffffu;
    int prev = 64; bool later = false;
#pragma unroll
    for (int j = 0; j < 64; j++) {
        const uint32_t pj = (uint32_t)__builtin_amdgcn_readlane((int)pos, j);
        if (pj == pos && j < lane) prev = j;
        if (pj == pos && j > lane) later = true;
    }
    if (valid) {
        pos16[(size_t)d * (size_t)B + (size_t)b] = (uint16_t)pos;
        meta8[(size_t)d * (size_t)B + (size_t)b] = (uint8_t)prev | (later ? 0u : 0x80u);
    }
}
}  // namespace

hipError_t launch_build_chains(hipStream_t s, uint16_t *d_pos16, uint8_t *d_meta8, int32_t num_bins, int depth, int width) {
    const int chunks = (num_bins + 63) / 64;
    hipLaunchKernelGGL(k_build_chains, dim3((chunks + 3) / 4, depth), dim3(256), 0, s, d_pos16, d_meta8, num_bins, width);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// hulk_step_sharded, delta exchange.  In the steady state of a stream (no element of the step can lower any weight on
// any rank: k_flush_decide's whole-batch bound, evaluated one step earlier) all a flush still changes is the count-min
// counters (countmin.go:122-127), the element count and the 1 % rule (kmerspectrum.go:84-96) — then it wipes the spectra
// (kmerspectrum.go:58-64).  A rank therefore reduces each of ITS intervals to the increments it causes:
//   k_shard_local : workgroup (bin segment, interval): waves 0..6 add the segment's counts to their row's 2000 counters
//                   in LDS (as k_cms_segsum), wave 7 counts the used bins; the workgroup adds its sums to the interval's
//                   delta vector (consecutive addresses: coalesced atomics) and wipes the segment.  One pass, one launch.
//   k_shard_apply : after the all-gather of every rank's {header, deltas}: thread per counter walks the intervals of the
//                   step in stream order — rank 0's, rank 1's, ... — applies flush_go()'s rule to each and adds.
// Unsigned integer sums: the counters equal those of the spectra exchange bit for bit.
// ------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(512) void k_shard_local(uint32_t *__restrict__ hists, const uint16_t *__restrict__ pos16,
                                                     uint32_t *__restrict__ hdr, uint32_t *__restrict__ delta, int depth,
                                                     int width, int seg_chunks, FlushBatch fb) {
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *lctr = (uint32_t *)smem;                           // [depth][width]
    const int seg = blockIdx.x, t = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, d = tid >> 6;  // waves 0..depth-1: rows; wave depth: used bins
    const size_t B = (size_t)fb.num_bins;
    uint32_t *hist = hists + (size_t)ring_slot(fb, t) * B;
    const int64_t b0 = (int64_t)seg * seg_chunks * 64;
    cms_seg_row_sums(lctr, hist, pos16, B, b0, depth, width, seg_chunks);
    if (d == depth) {
        unsigned cnt = 0;
        for (int c0 = 0; c0 < seg_chunks; c0++) {
            const int64_t b = b0 + (int64_t)c0 * 64 + lane;
            if (b < (int64_t)B) cnt += hist[b] != 0;
        }
        for (int off = 32; off; off >>= 1) cnt += __shfl_xor(cnt, off);
        if (lane == 0 && cnt) atomicAdd(&hdr[SHARD_USED + t], cnt);
    }
    __syncthreads();
    uint32_t *out = delta + (size_t)t * depth * width;
    for (int i = tid; i < depth * width; i += blockDim.x) { const uint32_t v = lctr[i]; if (v) atomicAdd(&out[i], v); }
    const int64_t w1 = b0 + (int64_t)seg_chunks * 64;
    for (int64_t b = b0 + tid; b < w1 && b < (int64_t)B; b += blockDim.x) hist[b] = 0;      // Wipe
}

__global__ __launch_bounds__(256) void k_shard_apply(const uint32_t *__restrict__ hdr_all, const uint32_t *__restrict__ delta_all,
                                                     unsigned long long *__restrict__ ctr, int ncounters, uint32_t world,
                                                     uint32_t T, uint32_t step_intervals, int32_t num_bins, DevState *st,
                                                     uint32_t step_tag) {
    // grid = (counters / 256, ranks): a workgroup adds ONE rank's intervals to its 256 counters (integer sums: the order of
    // the ranks' atomic adds does not matter); the rank's header words come in with one load per lane
    __shared__ uint32_t h[SHARD_HDR];
    const uint32_t r = blockIdx.y;
    if (threadIdx.x < SHARD_HDR) h[threadIdx.x] = hdr_all[(size_t)r * SHARD_HDR + threadIdx.x];
    __syncthreads();
    const uint32_t lo = r * T;                                                 // rank r holds intervals [r*T, r*T + cnt) of the step
    const uint32_t cnt = step_intervals <= lo ? 0u : (step_intervals - lo < T ? step_intervals - lo : T);
    // flush_go()'s rule per interval
    uint32_t gomask = 0; unsigned long long elems = 0; bool few = false;
    for (uint32_t t = 0; t < cnt; t++) {
        const uint32_t used = h[SHARD_USED + t];
        if (used == 0) continue;                                               // boss.go:118: nothing to flush
        if ((double)used / (double)num_bins < 0.01) { few = true; continue; }  // kmerspectrum.go:88-96 ("not used yet")
        gomask |= 1u << t;
        elems += used;
    }
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        if (h[SHARD_TAG] != step_tag) set_error(st, -37);                      // HULK_ERR_COMM: a block that is not of this step (the seal: hulk_comm.hip)
        if (few) set_error(st, -5);
        if (elems) atomicAdd(&st->n_elements, elems);
    }
    if (i >= ncounters || !gomask) return;
    const uint32_t *dr = delta_all + (size_t)r * T * (size_t)ncounters + i;
    uint32_t v[SCAN_BATCH_MAX];
#pragma unroll
    for (uint32_t t = 0; t < (uint32_t)SCAN_BATCH_MAX; t++) v[t] = (t < T && ((gomask >> t) & 1u)) ? dr[(size_t)t * ncounters] : 0u;   // all loads in flight
    unsigned long long sum = 0;
#pragma unroll
    for (uint32_t t = 0; t < (uint32_t)SCAN_BATCH_MAX; t++) sum += v[t];
    if (sum) atomicAdd(&ctr[i], sum);
}
// The gathered header of a step, on every rank: each block must be sealed with this step's tag.  `fatal` (delta exchange:
// the used-bin counts of a void block cannot be trusted and the spectra behind them are wiped) raises HULK_ERR_COMM; after
// a spectra exchange the header only carries the verdicts for the next step, which a void block turns into "full" on every
// rank (hulk_comm.hip).  The kernel itself stores the header to the host's mapped copy: no copy engine between the
// exchange and the host's view of it.
__global__ __launch_bounds__(256) void k_shard_check(const uint32_t *__restrict__ hdr_all, uint32_t world, uint32_t step_tag,
                                                     DevState *st, uint32_t *__restrict__ h_out, int fatal) {
    const uint32_t n = world * SHARD_HDR;
    bool bad = false;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t v = hdr_all[i];
        if ((i % SHARD_HDR) == SHARD_TAG && v != step_tag) bad = true;
        if (h_out) __builtin_nontemporal_store(v, &h_out[i]);
    }
    if (bad && fatal) set_error(st, -37);                                      // HULK_ERR_COMM
    __threadfence_system();
}
}  // namespace

hipError_t launch_shard_check(hipStream_t s, const uint32_t *d_hdr_all, uint32_t world, uint32_t step_tag, DevState *st,
                              uint32_t *h_out, int fatal) {
    prof_mark(s, "k_shard_check");
    hipLaunchKernelGGL(k_shard_check, dim3(1), dim3(256), 0, s, d_hdr_all, world, step_tag, st, h_out, fatal);
    return hipGetLastError();
}

hipError_t launch_shard_local(hipStream_t s, uint32_t *d_hists, const uint16_t *d_pos16, uint32_t *d_hdr, uint32_t *d_delta,
                              int depth, int width, const FlushBatch &fb) {
    if (fb.count == 0) return hipSuccess;
    const int seg_chunks = cms_seg_chunks(fb.num_bins);
    prof_mark(s, "k_shard_local");
    hipLaunchKernelGGL(k_shard_local, dim3(CMS_SEGS, fb.count), dim3(512), (size_t)depth * width * 4, s, d_hists, d_pos16, d_hdr,
                       d_delta, depth, width, seg_chunks, fb);
    return hipGetLastError();
}

hipError_t launch_shard_apply(hipStream_t s, const uint32_t *d_hdr_all, const uint32_t *d_delta_all, unsigned long long *d_ctr,
                              int depth, int width, uint32_t world, uint32_t T, uint32_t step_intervals, int32_t num_bins,
                              DevState *st, uint32_t step_tag) {
    const int nc = depth * width;
    const uint32_t ranks = std::min<uint32_t>(world, (step_intervals + T - 1) / T);      // ranks that hold intervals of this step
    prof_mark(s, "k_shard_apply");
    hipLaunchKernelGGL(k_shard_apply, dim3((nc + 255) / 256, ranks ? ranks : 1), dim3(256), 0, s, d_hdr_all, d_delta_all, d_ctr, nc,
                       world, T, step_intervals, num_bins, st, step_tag);
    return hipGetLastError();
}

}  // namespace hulk
