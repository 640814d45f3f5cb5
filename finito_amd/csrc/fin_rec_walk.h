// fin_rec_walk.h -- device code: the found stretches of a fast-path record, shared by the record consumers that want them as stretches (fin_segments.hip: one
// segment each; fin_readsum.hip: their number, their sum, the longest, first and last)
#pragma once
#include <stdint.h>

namespace {
// the found stretches [from, to) of a kind-1 record's strand slots, ascending: emit(ordinal, from, to); returns how many.  a = {u, off0, meta, nk}, b = the two
// position words (Es, Es2).  A position E makes slots [E - (k - 1), E] absent, clamped to [0, nk - 1]; a gap never starts below the end of its predecessor
// (done_to), exactly as fin_expand_records works them out: at most nine stretches.  nk > 0
template <class F>
__device__ __forceinline__ uint32_t sgm_rec_walk(const uint4 a, const uint4 b, uint32_t k, F&& emit) {
    const uint32_t nk = a.w, nE = min(a.z & 0xFFu, 8u), k1 = k - 1u;
    uint32_t done_to = 0, from = 0, n = 0;
#pragma unroll
    for (uint32_t e = 0; e < 8u; e++) {
        if (e < nE) {
            const uint32_t w = e < 2u ? b.x : e < 4u ? b.y : e < 6u ? b.z : b.w, E = (e & 1u) ? w >> 16 : w & 0xFFFFu;
            uint32_t lo = E >= k1 ? E - k1 : 0u;
            const uint32_t hi = E < nk ? E : nk - 1u;
            if (lo < done_to) lo = done_to;
            if (lo <= hi) {
                if (lo > from) { emit(n, from, lo); n++; }
                from = hi + 1u;
            }
            if (hi + 1u > done_to) done_to = hi + 1u;
        }
    }
    if (nk > from) { emit(n, from, nk); n++; }
    return n;
}
}  // namespace
