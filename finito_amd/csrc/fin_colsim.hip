// fin_colsim.hip -- SHARED K-MERS BETWEEN REFERENCES: the colour matrix times itself under a weight per unitig (include/finito_amd.h: fin_colors_shared;
// DESIGN.md 4.23).  B = the bit matrix uint64 bits[n_unitigs][W], v(u) one integer per unitig:
//   out[i][j] = the sum of v(u) over the unitigs u whose row R(u) has bit i and bit j,   0 <= i, j < n_colors,   mod 2^64
// the full symmetric uint64[n_colors][n_colors], row stride n_colors.  v(u) = vals[u], or (vals null) nk(u) = len(u) - k + 1 from the replica's ends (fin_nk.h).
//
// NO SCRATCH; NO LANE WAITS FOR ANOTHER LANE'S STORE; NO FLOATING POINT; every loop bound is a kernel argument or wave-uniform (a broadcast word, the block's
// number); integer atomics only, so every sum is exact in any order.
//   fin_colsim_tile_kernel    a wave (a block of 64) per (tile, chunk of unitigs); a tile is a pair of colour words wi <= wj.  The wave's own acc[64][64] of uint64
//                             is 32 KB of LDS: acc[a][l] is colour pair (64 wi + a, 64 wj + l), and column l belongs to lane l alone -- plain LDS read-add-writes of
//                             eight bytes at consecutive addresses, no LDS atomics, no bank conflicts, no barrier after the zeroing (a lane zeroes what it adds to).
//                             The chunk goes by in slices of 64 unitigs: lane l loads unitig (slice + l)'s word wi and, where that is not zero, its word wj, and the wave walks the
//                             lanes where both words are non-zero (a ballot), broadcasting the words and the value by readlane.  For a walked unitig the loop over
//                             the set bits a of word wi is scalar (the word is broadcast); lane l adds v to acc[a][l] where bit l of word wj is set.  The diagonal
//                             tiles wi == wj are no special case.  At the chunk's end the non-zero entries go out as 64-bit global atomic adds, a row of 64
//                             consecutive addresses at a time, into the upper triangle of tiles only.
//   fin_colsim_mirror_kernel  a wave per tile wi < wj, behind the tile kernel on the stream: out[j][i] = out[i][j], the stores coalesced.
// Bits at or above n_colors cannot be set (fin_colors_upload refuses them, the adds check `color`), so nothing is masked; rows and lanes behind n_colors store
// nothing all the same: out's stride is n_colors, not 64 W.
#include <algorithm>

#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_nk.h"
#include "fin_wave.h"

namespace {
typedef unsigned long long ull;

// tile t of the upper triangle, row by row: (0,0) (0,1) .. (0,W-1) (1,1) ..  At most W steps, on a value every lane shares
__device__ __forceinline__ void csm_tile(uint32_t t, uint32_t W, uint32_t& wi, uint32_t& wj) {
    wi = 0;
    while (t >= W - wi) { t -= W - wi; wi++; }
    wj = wi + t;
}
}  // namespace

// block b: tile b % n_tiles, chunk b / n_tiles (unitigs [chunk * c, ...)); chunk is a multiple of 64
__global__ __launch_bounds__(64) void fin_colsim_tile_kernel(const ull* bits, uint32_t n_unitigs, uint32_t W, uint32_t n_tiles, uint32_t chunk, uint32_t n_colors,
                                                             const uint32_t* ends_p, uint64_t total_len, uint32_t k, const ull* vals, ull* out) {
    __shared__ ull acc[64 * 64];
    const uint32_t lane = threadIdx.x;
    uint32_t wi, wj;
    csm_tile(blockIdx.x % n_tiles, W, wi, wj);
    const uint64_t u0 = (uint64_t)(blockIdx.x / n_tiles) * chunk;
    const uint32_t u1 = (uint32_t)std::min<uint64_t>(n_unitigs, u0 + chunk);
#pragma unroll 8
    for (uint32_t a = 0; a < 64u; a++) acc[a * 64u + lane] = 0ull;   // (lane l's column: nobody else reads or writes it before the end)
    bool any = false;
    for (uint32_t base = (uint32_t)u0; base < u1; base += 64u) {   // wave-uniform
        const uint32_t u = base + lane;
        const bool in = u < u1;
        const ull word_i = in ? bits[(uint64_t)u * W + wi] : 0ull;
        const ull word_j = word_i != 0ull ? bits[(uint64_t)u * W + wj] : 0ull;   // (a sparse row: most lanes have nothing to fetch)
        const bool mine = word_i != 0ull && word_j != 0ull;
        ull live = __ballot(mine);
        if (live == 0ull) continue;
        ull v = 0;
        if (mine) v = vals ? vals[u] : (ull)fin_unitig_nk(ends_p, u, n_unitigs, total_len, k);
        live = __ballot(v != 0ull);   // (a unitig of weight 0 adds nothing)
        for (; live; live &= live - 1ull) {
            const int src = __ffsll((long long)live) - 1;
            const ull a_bits = fin_bcast64(word_i, src), b_bits = fin_bcast64(word_j, src), bv = fin_bcast64(v, src);
            any = true;
            if ((b_bits >> lane) & 1ull)
                for (ull m = a_bits; m; m &= m - 1ull) {   // (the same trip count in every lane: a_bits is the wave's)
                    ull* const p = acc + (uint32_t)(__ffsll((long long)m) - 1) * 64u + lane;
                    *p += bv;
                }
        }
    }
    if (!any) return;   // wave-uniform: nothing was walked
    const uint32_t cj = 64u * wj + lane;
    for (uint32_t a = 0; a < 64u; a++) {
        const uint32_t ci = 64u * wi + a;
        if (ci >= n_colors) break;   // wave-uniform
        const ull s = acc[a * 64u + lane];
        if (s != 0ull && cj < n_colors) (void)__hip_atomic_fetch_add(out + (uint64_t)ci * n_colors + cj, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// block b: tile b of the W (W - 1) / 2 pairs wi < wj.  Lane l takes row 64 wi + l of the upper tile, an entry at a time, and stores it to column 64 wi + l of the
// lower tile's rows: the stores of a wave are 64 consecutive words
__global__ __launch_bounds__(64) void fin_colsim_mirror_kernel(ull* out, uint32_t W, uint32_t n_colors) {
    const uint32_t lane = threadIdx.x;
    uint32_t wi = 0, t = blockIdx.x;
    while (t >= W - 1u - wi) { t -= W - 1u - wi; wi++; }
    const uint32_t wj = wi + 1u + t;
    const uint32_t ci = 64u * wi + lane;   // (wi < wj <= W - 1: every ci is a colour)
    for (uint32_t r = 0; r < 64u; r++) {
        const uint32_t cj = 64u * wj + r;
        if (cj >= n_colors) break;   // wave-uniform
        out[(uint64_t)cj * n_colors + ci] = out[(uint64_t)ci * n_colors + cj];
    }
}

// unitigs per chunk: option "colsim_chunk" rounded up to a multiple of 64, or (0) 4096 and more once that would make over 16384 waves; never so few that the
// grid of tiles x chunks would pass 2^30 blocks
extern "C" uint32_t fin_colsim_chunk(uint64_t n_unitigs, uint32_t W, uint32_t colsim_chunk) {
    const uint64_t tiles = (uint64_t)std::max(W, 1u) * (std::max(W, 1u) + 1u) / 2u;
    uint64_t c = colsim_chunk;
    if (c == 0) {
        const uint64_t chunks = std::max<uint64_t>(1u, 16384u / tiles);
        c = std::max<uint64_t>(4096u, (n_unitigs + chunks - 1u) / chunks);
    }
    const uint64_t max_chunks = std::max<uint64_t>(1u, (1ull << 30) / tiles);
    c = std::max<uint64_t>(c, (n_unitigs + max_chunks - 1u) / max_chunks);
    return (uint32_t)((c + 63u) / 64u * 64u);
}

// out: uint64[n_colors][n_colors], zeroed here on `stream`.  vals (uint64[n_unitigs]) may be null: nk from ends_p, total_len and k
extern "C" int fin_launch_color_shared(const void* bits, uint32_t n_unitigs, uint32_t W, uint32_t n_colors, const uint32_t* ends_p, uint64_t total_len, uint32_t k,
                                       const void* vals, uint32_t colsim_chunk, uint64_t* out, hipStream_t stream) {
    if (W == 0 || W > 64u || n_colors == 0 || n_colors > 64u * W || n_colors + 64u <= 64u * W || n_unitigs >= 0x80000000u) return (int)hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(out, 0, (size_t)n_colors * n_colors * 8u, stream);
    if (e != hipSuccess) return (int)e;
    if (n_unitigs == 0) return 0;
    const uint32_t chunk = fin_colsim_chunk(n_unitigs, W, colsim_chunk), n_tiles = W * (W + 1u) / 2u;
    const uint64_t n_chunks = ((uint64_t)n_unitigs + chunk - 1u) / chunk;
    hipLaunchKernelGGL(fin_colsim_tile_kernel, dim3((uint32_t)(n_chunks * n_tiles)), dim3(64), 0, stream, (const ull*)bits, n_unitigs, W, n_tiles, chunk, n_colors, ends_p,
                       total_len, k, (const ull*)vals, (ull*)out);   // (at most 2^30 blocks: fin_colsim_chunk)
    e = hipGetLastError();
    if (e != hipSuccess || W == 1u) return (int)e;
    hipLaunchKernelGGL(fin_colsim_mirror_kernel, dim3(W * (W - 1u) / 2u), dim3(64), 0, stream, (ull*)out, W, n_colors);
    return (int)hipGetLastError();
}
