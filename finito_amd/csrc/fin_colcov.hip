// fin_colcov.hip -- BREADTH AND DEPTH OF COVERAGE PER REFERENCE: the per-unitig numbers of the coverage line projected through the colour matrix
// (include/finito_amd.h: fin_colors_coverage).  Per unitig u, four values, exact integers:
//   v(u) = {nk(u) = len(u) - k + 1, cov(u) = covered[u], sum(u) = stats[u].sum, sol(u) = stats[u].n_at_least}      (covered / stats null: 0)
// Out, per colour c: out[c] = {kmers, kmers_only, covered, covered_only, depth_sum, depth_sum_only, solid, solid_only} -- v summed over the unitigs whose row
// R(u) has bit c, and (the _only fields) over those whose row is {c}.  none[8]: v summed over the unitigs with an empty row, in the same places (its _only
// fields stay 0).  A bit-matrix-transpose times an integer matrix.
//
// NO SCRATCH; NO LANE WAITS FOR ANOTHER LANE'S STORE; every loop bound is a kernel argument; integer atomics only, so every sum is exact in any order.
//   fin_colcov_class_kernel   cls[u] = 0 (R(u) empty), 1 (one bit) or 2 (more): a group of S lanes per unitig, S = the power of two >= W (at most 64), lane i of
//                             the group words i, i + S, ...: the row load is coalesced at every W; the popcounts meet in a butterfly over the group.  The empty
//                             rows' values are summed per wave and go to none[] as four atomics per wave that has any.  With the byte the column kernel never
//                             needs the whole row.
//   fin_colcov_column_kernel  a wave per (colour word w, chunk of unitigs): lane j is colour 64 w + j and keeps the eight sums in registers.  The chunk goes by
//                             in slices of 64 unitigs.  LOADS = 0: lane l loads unitig (slice + l)'s word, class and values, one load each per slice, and the
//                             wave walks the lanes whose word is not zero (a ballot), broadcasting word, class and values by readlane -- a slice of empty
//                             words costs its loads and one ballot.  LOADS = 1: every lane loads the same unitig's word, class and values (wave-uniform
//                             addresses), unitig by unitig.  Each lane adds where its bit is set, and to the _only sums where the class is 1 as well.  At the
//                             chunk's end a lane with anything to add does eight (or fewer) 64-bit global atomic adds.  Four waves of a block take four
//                             neighbouring words of the same chunk, and the block number runs over the word groups first: the 32 bytes a wave takes of a
//                             row's line are taken by its neighbours at the same time.
// Bits at or above n_colors cannot be set (fin_colors_upload refuses them, the adds check `color`), so nothing is masked: the lanes behind n_colors add nothing.
#include <algorithm>

#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_nk.h"
#include "fin_wave.h"

#define FIN_CCV_BLK 256u

namespace {
typedef unsigned long long ull;

__device__ __forceinline__ void ccv_add(ull* p, ull v) {
    if (v) (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
}  // namespace

// S lanes per unitig (a power of two, 1 .. 64, >= W or 64); 256 / S unitigs per block
__global__ __launch_bounds__(256) void fin_colcov_class_kernel(const ull* bits, uint32_t n_unitigs, uint32_t W, uint32_t S, const uint32_t* ends_p, uint64_t total_len,
                                                               uint32_t k, const ull* covered, const FinDepthStat* stats, uint8_t* cls, ull* none) {
    const uint32_t per_block = FIN_CCV_BLK / S;
    const uint64_t u64 = (uint64_t)blockIdx.x * per_block + threadIdx.x / S;
    const uint32_t sub = threadIdx.x & (S - 1u);
    const bool in = u64 < n_unitigs;
    const uint32_t u = in ? (uint32_t)u64 : 0u;
    uint32_t pc = 0;
    if (in) for (uint32_t w = sub; w < W; w += S) pc += (uint32_t)__popcll(bits[(uint64_t)u * W + w]);
    for (uint32_t s = S >> 1; s >= 1u; s >>= 1) pc += (uint32_t)__shfl_xor((int)pc, (int)s);   // (S is a kernel argument: the same trip count in every lane)
    const bool lead = in && sub == 0u;
    if (lead) cls[u] = (uint8_t)(pc < 2u ? pc : 2u);
    const bool empty = lead && pc == 0u;
    if (__ballot(empty) == 0ull) return;   // wave-uniform
    ull v0 = 0, v1 = 0, v2 = 0, v3 = 0;
    if (empty) {
        v0 = fin_unitig_nk(ends_p, u, n_unitigs, total_len, k);
        if (covered) v1 = covered[u];
        if (stats) { v2 = stats[u].sum; v3 = stats[u].n_at_least; }
    }
    v0 = fin_wave_sum64(v0); v1 = fin_wave_sum64(v1); v2 = fin_wave_sum64(v2); v3 = fin_wave_sum64(v3);
    if ((threadIdx.x & 63u) == 0u) { ccv_add(none + 0, v0); ccv_add(none + 2, v1); ccv_add(none + 4, v2); ccv_add(none + 6, v3); }
}

// block b: word group b % n_groups (words 4 g + wave), chunk b / n_groups (unitigs [chunk * c, ...)); chunk is a multiple of 64
template <int LOADS>
__global__ __launch_bounds__(256) void fin_colcov_column_kernel(const ull* bits, uint32_t n_unitigs, uint32_t W, uint32_t n_groups, uint32_t chunk, uint32_t n_colors,
                                                                const uint8_t* cls, const uint32_t* ends_p, uint64_t total_len, uint32_t k, const ull* covered,
                                                                const FinDepthStat* stats, ull* out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (blockIdx.x % n_groups) * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= W) return;   // wave-uniform
    const uint64_t u0 = (uint64_t)(blockIdx.x / n_groups) * chunk;
    const uint32_t u1 = (uint32_t)std::min<uint64_t>(n_unitigs, u0 + chunk);
    ull a_k = 0, a_ko = 0, a_c = 0, a_co = 0, a_s = 0, a_so = 0, a_n = 0, a_no = 0;
    if (LOADS == 0) {
        for (uint32_t base = (uint32_t)u0; base < u1; base += 64u) {   // wave-uniform
            const uint32_t u = base + lane;
            const bool in = u < u1;
            const ull word = in ? bits[(uint64_t)u * W + w] : 0ull;
            ull live = __ballot(word != 0ull);
            if (live == 0ull) continue;
            uint32_t c = 0, nk = 0, sol = 0;
            ull cv = 0, sum = 0;
            if (word != 0ull) {
                c = cls[u];
                nk = fin_unitig_nk(ends_p, u, n_unitigs, total_len, k);
                if (covered) cv = covered[u];
                if (stats) { sum = stats[u].sum; sol = stats[u].n_at_least; }
            }
            for (; live; live &= live - 1ull) {
                const int src = __ffsll((long long)live) - 1;
                const ull wd = fin_bcast64(word, src);
                const bool only = fin_bcast(c, src) == 1u;
                const ull b_nk = fin_bcast(nk, src), b_cv = fin_bcast64(cv, src), b_sum = fin_bcast64(sum, src), b_sol = fin_bcast(sol, src);
                if ((wd >> lane) & 1ull) {
                    a_k += b_nk; a_c += b_cv; a_s += b_sum; a_n += b_sol;
                    if (only) { a_ko += b_nk; a_co += b_cv; a_so += b_sum; a_no += b_sol; }
                }
            }
        }
    } else {
        for (uint32_t u = (uint32_t)u0; u < u1; u++) {   // wave-uniform, and so is every address below
            const ull wd = bits[(uint64_t)u * W + w];
            if (wd == 0ull) continue;
            const bool only = cls[u] == 1u;
            const ull b_nk = fin_unitig_nk(ends_p, u, n_unitigs, total_len, k), b_cv = covered ? covered[u] : 0ull, b_sum = stats ? stats[u].sum : 0ull,
                      b_sol = stats ? stats[u].n_at_least : 0u;
            if ((wd >> lane) & 1ull) {
                a_k += b_nk; a_c += b_cv; a_s += b_sum; a_n += b_sol;
                if (only) { a_ko += b_nk; a_co += b_cv; a_so += b_sum; a_no += b_sol; }
            }
        }
    }
    const uint32_t color = 64u * w + lane;
    if (color >= n_colors) return;   // (such a lane has added nothing: the bit cannot be set)
    ull* const o = out + (uint64_t)color * 8u;
    ccv_add(o + 0, a_k); ccv_add(o + 1, a_ko); ccv_add(o + 2, a_c); ccv_add(o + 3, a_co);
    ccv_add(o + 4, a_s); ccv_add(o + 5, a_so); ccv_add(o + 6, a_n); ccv_add(o + 7, a_no);
}

// unitigs per chunk: option "colcov_chunk" rounded up to a multiple of 64, or (0) 1024 and more once that would make over 8192 waves; never so few that there
// would be over 2^20 chunks
extern "C" uint32_t fin_colcov_chunk(uint64_t n_unitigs, uint32_t W, uint32_t colcov_chunk) {
    uint64_t c = colcov_chunk;
    if (c == 0) {
        const uint64_t chunks = std::max<uint64_t>(1u, 8192u / std::max(W, 1u));
        c = std::max<uint64_t>(1024u, (n_unitigs + chunks - 1u) / chunks);
    }
    c = std::max<uint64_t>(c, (n_unitigs + (1u << 20) - 1u) >> 20);
    return (uint32_t)((c + 63u) / 64u * 64u);
}

// the class byte alone, for a caller that projects something else through the matrix (fin_depthhist.hip): cls[u] = 0, 1 or 2 as above, by fin_colcov_class_kernel
// as it stands.  none8: eight uint64 of device scratch the kernel adds the empty rows' k-mers to (zeroed here; not a result)
extern "C" int fin_launch_color_classes(const void* bits, uint32_t n_unitigs, uint32_t W, const uint32_t* ends_p, uint64_t total_len, uint32_t k, void* cls, uint64_t* none8,
                                        hipStream_t stream) {
    if (W == 0 || W > 64u || n_unitigs >= 0x80000000u) return (int)hipErrorInvalidValue;
    if (n_unitigs == 0) return 0;
    const hipError_t e = hipMemsetAsync(none8, 0, 64u, stream);
    if (e != hipSuccess) return (int)e;
    uint32_t S = 1;
    while (S < W) S <<= 1;
    const uint32_t per_block = FIN_CCV_BLK / S;
    hipLaunchKernelGGL(fin_colcov_class_kernel, dim3((n_unitigs + per_block - 1u) / per_block), dim3(FIN_CCV_BLK), 0, stream, (const ull*)bits, n_unitigs, W, S, ends_p,
                       total_len, k, (const ull*)nullptr, (const FinDepthStat*)nullptr, (uint8_t*)cls, (ull*)none8);
    return (int)hipGetLastError();
}

// out: uint64[n_colors][8], none: uint64[8], both zeroed here on `stream`; cls: n_unitigs bytes, written here.  covered (uint64[n_unitigs]) and stats
// (FinDepthStat[n_unitigs]) may be null.  loads: 0, the coalesced slices (what the library uses), or 1, wave-uniform loads (tools/ab_colcov.py compares them)
extern "C" int fin_launch_color_coverage(const void* bits, uint32_t n_unitigs, uint32_t W, uint32_t n_colors, const uint32_t* ends_p, uint64_t total_len, uint32_t k,
                                         const void* covered, const void* stats, void* cls, uint32_t colcov_chunk, uint32_t loads, uint64_t* out, uint64_t* none,
                                         hipStream_t stream) {
    if (W == 0 || W > 64u || n_colors == 0 || n_colors > 64u * W || n_colors + 64u <= 64u * W || n_unitigs >= 0x80000000u || loads > 1u) return (int)hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(out, 0, (size_t)n_colors * 64u, stream);
    if (e == hipSuccess) e = hipMemsetAsync(none, 0, 64u, stream);
    if (e != hipSuccess) return (int)e;
    if (n_unitigs == 0) return 0;
    uint32_t S = 1;
    while (S < W) S <<= 1;
    const uint32_t per_block = FIN_CCV_BLK / S;
    hipLaunchKernelGGL(fin_colcov_class_kernel, dim3((n_unitigs + per_block - 1u) / per_block), dim3(FIN_CCV_BLK), 0, stream, (const ull*)bits, n_unitigs, W, S, ends_p,
                       total_len, k, (const ull*)covered, (const FinDepthStat*)stats, (uint8_t*)cls, (ull*)none);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const uint32_t chunk = fin_colcov_chunk(n_unitigs, W, colcov_chunk), n_groups = (W + 3u) / 4u;
    const uint64_t n_chunks = ((uint64_t)n_unitigs + chunk - 1u) / chunk;
    const dim3 grid((uint32_t)(n_chunks * n_groups));   // (at most 2^20 chunks of 16 groups)
    if (loads == 0)
        hipLaunchKernelGGL(fin_colcov_column_kernel<0>, grid, dim3(FIN_CCV_BLK), 0, stream, (const ull*)bits, n_unitigs, W, n_groups, chunk, n_colors, (const uint8_t*)cls,
                           ends_p, total_len, k, (const ull*)covered, (const FinDepthStat*)stats, (ull*)out);
    else
        hipLaunchKernelGGL(fin_colcov_column_kernel<1>, grid, dim3(FIN_CCV_BLK), 0, stream, (const ull*)bits, n_unitigs, W, n_groups, chunk, n_colors, (const uint8_t*)cls,
                           ends_p, total_len, k, (const ull*)covered, (const FinDepthStat*)stats, (ull*)out);
    return (int)hipGetLastError();
}
