// fin_absum.h -- the ORDER of a row's sum of per-colour doubles, stated once (device only): fin_abundance.hip's d_j and fin_assign.hip's d are the same number
// because both come from these two.  s_w = x over the set bits of word w in ascending bit order, starting from 0.0; the words' sums are then folded in halves,
// v = v[:h] + v[h:], over the power of two at or above W -- a butterfly over that many lanes, lane w holding s_w (0.0 behind W).
#pragma once
#include "fin_device.h"

// the sum over lanes 0 .. width - 1 (a power of two <= 64), the same in each of them: the order is the butterfly's, whatever the values
__device__ __forceinline__ double ab_butterfly(double v, uint32_t width) {
    for (uint32_t d = width >> 1; d >= 1u; d >>= 1) v += __shfl_xor(v, (int)d);
    return v;
}
__device__ __forceinline__ double ab_bits_sum(unsigned long long word, const double* x64) {   // x over the word's set bits, ascending
    double s = 0.0;
    for (; word; word &= word - 1ull) s += x64[__ffsll((long long)word) - 1];
    return s;
}
