// fin_rowhash.h -- the 64-bit hash of a colour row, shared by the equivalence-class table (fin_eqclasses.hip: its tag is this hash narrowed), the bootstrap's
// generator (fin_bootstrap.hip: the counter holds it whole) and the bootstrap's host twin (fin_capi.cpp): h = the xor over the words i < W of
// ec_word_hash(word_i, i).  Commutative over the words, so a wave may hold a word per lane and reduce with xor.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FIN_HD __host__ __device__ __forceinline__
#else
#define FIN_HD static inline
#endif

FIN_HD uint64_t ec_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// word i's share of the row's hash: the row's hash is the xor of its words' shares
FIN_HD uint64_t ec_word_hash(uint64_t word, uint32_t i) { return ec_mix(word + (uint64_t)(i + 1u) * 0x9E3779B97F4A7C15ull); }

#if defined(__HIPCC__)
__device__ __forceinline__ uint64_t ec_wave_xor(uint64_t v) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { lo ^= (uint32_t)__shfl_xor((int)lo, d); hi ^= (uint32_t)__shfl_xor((int)hi, d); }
    return ((uint64_t)hi << 32) | lo;
}
#endif
