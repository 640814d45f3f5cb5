// fin_rec_walk.h -- THE statement of the record gap rule, for the device and the host alike: what a fast-path record (FinFastRec, fin_read_record) means is
// worked out here and nowhere else.  Every consumer of records takes the gaps (fin_rec_gaps) or their complement, the found stretches (fin_rec_stretches):
// fin_hits.hip, fin_cover.hip, fin_depth.hip, fin_pileup.hip, fin_segments.hip, fin_readsum.hip, fin_classify.hip, fin_colors.hip, fin_paired.hip and the host twins of
// fin_records_host.cpp.  What a device consumer does AROUND the walk -- which reads have a record, the wave's turn through the searched ones, a read's rows --
// is fin_wave.h's.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FIN_HD __host__ __device__ __forceinline__
#define FIN_UNROLL _Pragma("unroll")
#else
#define FIN_HD static inline
#define FIN_UNROLL
#endif

// The rule.  A kind-1 record has nk strand slots and nE (at most 8) disagreeing positions, ascending, 16 bits each in the words w0 .. w3 (the device's b.x .. b.w,
// the halves of the host's Es and Es2).  A position E makes slots [E - (k - 1), E] absent, clamped to [0, nk - 1]; gaps may touch or overlap, so a gap never starts
// below the end of its predecessor (done_to).  emit(lo, hi_excl) per gap: non-empty, ascending, disjoint.  nk == 0 gives none
template <class F>
FIN_HD void fin_rec_gaps(uint32_t nk, uint32_t nE, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t k, F&& emit) {
    if (nk == 0u) return;
    const uint32_t k1 = k - 1u;
    uint32_t done_to = 0;
    FIN_UNROLL
    for (uint32_t e = 0; e < 8u; e++) {
        if (e < nE) {
            const uint32_t w = e < 2u ? w0 : e < 4u ? w1 : e < 6u ? w2 : w3, E = (e & 1u) ? w >> 16 : w & 0xFFFFu;
            uint32_t lo = E >= k1 ? E - k1 : 0u;
            const uint32_t hi = E < nk ? E : nk - 1u;
            if (lo < done_to) lo = done_to;
            if (lo <= hi) emit(lo, hi + 1u);
            if (hi + 1u > done_to) done_to = hi + 1u;
        }
    }
}

// The found stretches [from, to) of the record's strand slots, ascending -- what the gaps leave of [0, nk): emit(ordinal, from, to); returns how many, at most nine
template <class F>
FIN_HD uint32_t fin_rec_stretches(uint32_t nk, uint32_t nE, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t k, F&& emit) {
    uint32_t from = 0, n = 0;
    fin_rec_gaps(nk, nE, w0, w1, w2, w3, k, [&](uint32_t lo, uint32_t hi_excl) {
        if (lo > from) { emit(n, from, lo); n++; }
        from = hi_excl;
    });
    if (nk > from) { emit(n, from, nk); n++; }
    return n;
}

#if defined(__HIPCC__)
// ... of a record as a lane holds it: a = {u, off0, meta, nk}, b = the position words
template <class F>
__device__ __forceinline__ uint32_t sgm_rec_walk(const uint4 a, const uint4 b, uint32_t k, F&& emit) {
    return fin_rec_stretches(a.w, a.z & 0xFFu, b.x, b.y, b.z, b.w, k, emit);
}

// a step whose overflow list overran has no results (batch_overrun_check, fin_capi.cpp): the consumer writes nothing of it, bit 0 of its flag word is set
__device__ __forceinline__ bool fin_step_withheld(const uint32_t* ovf_count, uint32_t ovf_cap, uint32_t* flags) {
    if (!ovf_count || *ovf_count <= ovf_cap) return false;
    if (blockIdx.x == 0 && threadIdx.x == 0) (void)__hip_atomic_fetch_or(flags, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}
#endif
