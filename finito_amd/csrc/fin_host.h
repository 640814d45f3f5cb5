// fin_host.h -- host helpers shared by fin_capi.cpp and the host twins of fin_records_host.cpp.  Plain C++: no HIP header
#pragma once
#include <stdint.h>

// the first unitig of a colour matrix bits[n_unitigs][W] with a bit at or above n_colors set, or n_unitigs
static inline uint64_t colors_first_stray(const uint64_t* bits, uint64_t n_unitigs, uint32_t n_colors, uint32_t W) {
    if ((n_colors & 63u) == 0u) return n_unitigs;   // (the last word is all colours)
    const uint64_t stray = ~0ull << (n_colors & 63u);
    for (uint64_t u = 0; u < n_unitigs; u++) if (bits[u * W + (W - 1)] & stray) return u;
    return n_unitigs;
}
