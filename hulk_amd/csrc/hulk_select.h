// hulk_select.h — the running list of the K best candidates that k_search_select (hulk_search.hip) and k_index_select (hulk_index.hip)
// keep: one rule in one place.  A wave owns a query; lane l < K holds entry l of its list (kd: the distance's bits, ki: the database
// index), ascending by the 96-bit key (kd, ki) — a non-negative, non-NaN double orders like its uint64 bits; unused entries are
// ~0 / ~0, behind every key a pair can have.  (td, ti) is the K-th key in every lane: what a candidate has to beat.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hulk {

__device__ __forceinline__ bool select_beats(unsigned long long bits, uint32_t gi, unsigned long long td, uint32_t ti) {
    return bits < td || (bits == td && gi < ti);
}

// mask: the lanes whose candidate (bits, gi) passed its tests and select_beats at the time of the ballot.  They are taken in lane
// order and inserted: a candidate's rank in the list is a ballot's population count, the tail moves up one lane.  The compare is the
// full key, so the list is a function of the set of candidates alone
__device__ __forceinline__ void select_insert(unsigned long long mask, unsigned long long bits, uint32_t gi, uint32_t lane, uint32_t K,
                                              unsigned long long &kd, uint32_t &ki, unsigned long long &td, uint32_t &ti) {
    while (mask) {
        const int src = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const unsigned long long cd = __shfl(bits, src);
        const uint32_t ci = __shfl(gi, src);
        if (!select_beats(cd, ci, td, ti)) continue;                // (the K-th key has moved since the ballot)
        const bool less = lane < K && (kd < cd || (kd == cd && ki < ci));
        const uint32_t pos = (uint32_t)__popcll(__ballot(less));    // < K: the candidate beats the K-th key
        const unsigned long long ud = __shfl_up(kd, 1);
        const uint32_t ui = __shfl_up(ki, 1);
        if (lane > pos) { kd = ud; ki = ui; }
        else if (lane == pos) { kd = cd; ki = ci; }
        td = __shfl(kd, (int)K - 1);
        ti = __shfl(ki, (int)K - 1);
    }
}

}  // namespace hulk
