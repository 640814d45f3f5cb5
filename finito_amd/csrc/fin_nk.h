// fin_nk.h -- the k-mers of a unitig from the replica's ends, stated once (device only): fin_colcov.hip's and fin_colsim.hip's default value per unitig.
#pragma once
#include "fin_device.h"

// nk(u) = len(u) - k + 1: ends_p[u] is the start of unitig u and ends_p[u + 1] its exclusive end; the last unitig ends at total_len
__device__ __forceinline__ uint32_t fin_unitig_nk(const uint32_t* ends_p, uint32_t u, uint32_t n_unitigs, uint64_t total_len, uint32_t k) {
    const uint64_t s = ends_p[u], e = u + 1u < n_unitigs ? (uint64_t)ends_p[u + 1u] : total_len;
    return e >= s + k ? (uint32_t)(e - s - k + 1u) : 0u;
}
