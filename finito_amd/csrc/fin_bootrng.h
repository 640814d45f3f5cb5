// fin_bootrng.h -- the bootstrap's draws, one statement for the device (fin_bootstrap.hip) and the host twin (fin_capi.cpp).
// Philox4x32-10 with the standard constants; key {seed low, seed high}; block i of the class with row hash h in replicate b has the counter
// {h low, h high, i low 32, (i >> 32) | (b << 8)} (i < 2^38 since n_j < 2^40, b < 4096), and output word m of block i belongs to read 4 i + m of the class.
// A read's multiplicity is X(u) = the number of k in 0 .. 12 with u >= T_k, T_k = floor(2^32 e^-1 sum_{i <= k} 1 / i!): Poisson(1) quantised to 2^-32, at most 13.
#pragma once
#include <stdint.h>

#include "fin_rowhash.h"

#define FIN_BOOT_SLAB 4096u          // reads per slab: 1024 Philox blocks, 16 per lane of the wave that takes the slab
#define FIN_BOOT_MAX 4096u           // replicates per call
// N n_boot of one call.  Measured on an MI355X (profiles/r26/bootstrap.md): 31.6 G draws/s with 100 reads per class, so 2^38 draws take 8.7 s over the whole call;
// with 10 reads per class the kernel is bound by its slabs (3.1 ns each), not by the draws.  One launch has at most N / 4096 + C <= 2^27 slabs: about 0.4 s
#define FIN_BOOT_MAX_DRAWS (1ull << 38)

FIN_HD void fin_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// block i of class hash h, replicate b
FIN_HD void fin_boot_block(uint64_t h, uint64_t i, uint32_t b, uint64_t seed, uint32_t out[4]) {
    fin_philox4x32_10((uint32_t)h, (uint32_t)(h >> 32), (uint32_t)i, (uint32_t)(i >> 32) | (b << 8), (uint32_t)seed, (uint32_t)(seed >> 32), out);
}
FIN_HD uint32_t fin_boot_mult(uint32_t u) {
    return (uint32_t)(u >= 0x5e2d58d8u) + (uint32_t)(u >= 0xbc5ab1b1u) + (uint32_t)(u >= 0xeb715e1du) + (uint32_t)(u >= 0xfb239797u) + (uint32_t)(u >= 0xff1025f5u) +
           (uint32_t)(u >= 0xffd90f3bu) + (uint32_t)(u >= 0xfffa8b71u) + (uint32_t)(u >= 0xffff540cu) + (uint32_t)(u >= 0xffffed1fu) + (uint32_t)(u >= 0xfffffe21u) +
           (uint32_t)(u >= 0xffffffd4u) + (uint32_t)(u >= 0xfffffffcu) + (uint32_t)(u >= 0xffffffffu);
}
// the multiplicities of block i's reads below n (n > 4 i), summed
FIN_HD uint32_t fin_boot_block_sum(uint64_t h, uint64_t i, uint64_t n, uint32_t b, uint64_t seed) {
    uint32_t o[4];
    fin_boot_block(h, i, b, seed, o);
    const uint64_t left = n - 4ull * i;
    uint32_t s = fin_boot_mult(o[0]);
    if (left > 1ull) s += fin_boot_mult(o[1]);
    if (left > 2ull) s += fin_boot_mult(o[2]);
    if (left > 3ull) s += fin_boot_mult(o[3]);
    return s;
}
