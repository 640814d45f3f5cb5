// fin_depthhist.hip -- DEPTH HISTOGRAMS: the k-mer spectrum of a run and the histogram of every reference's k-mer depths, made from the staged depths of
// fin_depth.hip's prefix sum (include/finito_amd.h: fin_depth_histogram, fin_colors_depth_histogram).  Integers throughout:
//   bin(d) = min(d / bin_width, n_bins - 1), 1 <= n_bins <= 1024, bin_width >= 1; a position g of unitig u COUNTS iff a k-mer begins there,
//   g - start(u) < nk(u), which is g + k <= end(u): the last k - 1 positions of a unitig never count, whatever their depth says.
//
// NO SCRATCH; NO LANE WAITS FOR ANOTHER LANE'S STORE; every loop bound is a kernel argument; integer atomics only, so every sum is exact in any order.
//   fin_dh_spectrum_kernel  hist[b] += the counted positions of one staged chunk whose depth falls into bin b.  fin_depth_stat_kernel's frame: a lane takes
//                           FIN_DH_P = 8 consecutive positions (two 16-byte loads), finds the first one's unitig by binary search in ends_p and walks on from
//                           there.  Depth is piecewise constant along a unitig, so a lane combines RUNS of equal bin and adds a run's length, not ones.  A block
//                           keeps n_bins uint32 counters in LDS (at most 4 KB; a block sees 2048 positions) and adds the non-zero ones to the global uint64
//                           table at its end, one 64-bit atomic each.
//       THE HOT BIN.  On a real run nearly every lane of a wave ends with one run of eight positions in bin 0 or in the modal bin: 64 LDS atomics on one
//       address, which the LDS takes one after the other.  A lane's LAST run -- the only one most lanes have -- therefore goes through a wave-uniform test
//       first: one ballot says whether every lane that holds a run holds the same bin; if so the lengths meet in a butterfly and one lane adds once.  A wave
//       that fails the test has paid one readlane and one ballot and adds lane by lane.  Runs a lane closes before its last one (the depth changed inside its eight
//       positions) are rare and go to LDS directly.  A sort or a per-wave private table was not considered worth its LDS: the uniform case is the common one.
//   fin_dh_unitig_kernel    the same frame over a window [lo, hi) of the stage that holds the positions of the unitigs [u_lo, u_hi): V[u - u_lo][b] += a run's
//                           length, one global 32-bit atomic per run of equal (unitig, bin), and one per wave where every lane's last run has the same unitig
//                           and bin.  Lanes stand on aligned groups of eight whatever lo is, so the 16-byte loads stay aligned; positions outside the window
//                           are skipped.
//   fin_dh_project_kernel   out[c][0 / 1][b] += the sum of V[u][b] over the unitigs of [u_lo, u_hi) whose row has bit c / is {c} alone: fin_colcov_column_kernel<0>'s
//                           walk with FIN_DH_S = 16 bins per unitig instead of four values.  A wave per (colour word, slice of 16 bins, chunk of unitigs): lane
//                           j is colour 64 w + j and keeps the slice's 16 "all" and 16 "only" sums in registers, uint32 -- V was binned from fewer than 2^32
//                           positions (the launcher checks), so no column of it sums past that.  The chunk goes by in slices of 64 unitigs: lane l loads
//                           unitig (slice + l)'s word and class byte, the wave walks the lanes whose word is not zero and reads that unitig's 16 entries of V
//                           at wave-uniform addresses.  Cost follows the non-empty words, not the unitigs.  At the end a lane does at most 32 64-bit atomics.
//   fin_dh_none_kernel      none[b] += the sum of V[u][b] over the unitigs whose class byte is 0: a thread per bin, V read coalesced, the byte wave-uniform.
// The class byte is fin_colcov_class_kernel's (fin_launch_color_classes, fin_colcov.hip), made once per call.
#include <algorithm>

#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_wave.h"

#define FIN_DH_P 8u     // positions a lane takes (FIN_DEPTH_STAT_P's)
#define FIN_DH_S 16u    // bins a wave of the projection keeps per colour
#define FIN_DH_MAX_BINS 1024u

namespace {
typedef unsigned long long ull;

__device__ __forceinline__ void dh_add64(ull* p, ull v) {
    if (v) (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a lane's last run {u, b, len} (len 0: none) after it has handed every earlier one to flush(u, b, len).  depth[0 .. n) are the depths of text positions g_base
// .. g_base + n; only the positions [lo, hi) of it are looked at.  BY_UNITIG: a run ends where the unitig does
template <bool BY_UNITIG, class F>
__device__ __forceinline__ void dh_walk(const uint32_t* depth, uint64_t g_base, uint64_t n, uint64_t lo, uint64_t hi, const uint32_t* ends_p, uint32_t n_unitigs,
                                        uint64_t total_len, uint32_t k, uint32_t n_bins, uint32_t bin_width, uint32_t& r_u, uint32_t& r_b, uint32_t& r_len, F&& flush) {
    r_u = 0; r_b = 0; r_len = 0;
    const uint64_t i0 = ((lo / FIN_DH_P) + (uint64_t)blockIdx.x * 256u + threadIdx.x) * FIN_DH_P;
    if (i0 >= hi) return;
    uint32_t d[FIN_DH_P];
    if (i0 + FIN_DH_P <= n) {   // (depth is 16-byte aligned and i0 a multiple of 8)
        const uint4 w0 = ((const uint4*)(depth + i0))[0], w1 = ((const uint4*)(depth + i0))[1];
        d[0] = w0.x; d[1] = w0.y; d[2] = w0.z; d[3] = w0.w; d[4] = w1.x; d[5] = w1.y; d[6] = w1.z; d[7] = w1.w;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < FIN_DH_P; j++) d[j] = i0 + j < n ? depth[i0 + j] : 0u;
    }
    const uint64_t g0 = g_base + i0;
    uint32_t a = 0, z = n_unitigs;   // the last u in [0, n_unitigs) with ends_p[u] <= g0 (ends_p[0] = 0)
    while (z - a > 1u) { const uint32_t mid = a + (z - a) / 2u; if ((uint64_t)ends_p[mid] <= g0) a = mid; else z = mid; }
    uint32_t u = a;
    uint64_t next = u + 1u < n_unitigs ? (uint64_t)ends_p[u + 1u] : total_len;   // the exclusive end of unitig u
    const uint32_t top = n_bins - 1u;
#pragma unroll
    for (uint32_t j = 0; j < FIN_DH_P; j++) {
        const uint64_t i = i0 + j;
        if (i >= lo && i < hi) {
            const uint64_t g = g_base + i;
            while (g >= next && u + 1u < n_unitigs) { u++; next = u + 1u < n_unitigs ? (uint64_t)ends_p[u + 1u] : total_len; }
            if (g + k <= next) {   // a k-mer begins at g
                const uint32_t q = bin_width == 1u ? d[j] : d[j] / bin_width;
                const uint32_t b = q < top ? q : top;
                if (r_len != 0u && (b != r_b || (BY_UNITIG && u != r_u))) { flush(r_u, r_b, r_len); r_len = 0u; }
                r_u = u; r_b = b; r_len++;
            }
        }
    }
}

// does every lane of the wave that holds a run hold the run {*u0, *b0}?  (wave-converged; false when no lane holds one)
template <bool BY_UNITIG>
__device__ __forceinline__ bool dh_uniform(uint32_t r_u, uint32_t r_b, uint32_t r_len, uint32_t* u0, uint32_t* b0) {
    const ull has = __ballot(r_len != 0u);
    if (has == 0ull) return false;
    const int src = __ffsll((long long)has) - 1;
    *u0 = fin_bcast(r_u, src); *b0 = fin_bcast(r_b, src);
    return __ballot(r_len != 0u && (r_b != *b0 || (BY_UNITIG && r_u != *u0))) == 0ull;
}
}  // namespace

__global__ __launch_bounds__(256) void fin_dh_spectrum_kernel(const uint32_t* depth, uint64_t g_base, uint64_t n, const uint32_t* ends_p, uint32_t n_unitigs,
                                                              uint64_t total_len, uint32_t k, uint32_t n_bins, uint32_t bin_width, ull* hist) {
    __shared__ uint32_t cnt[FIN_DH_MAX_BINS];
    for (uint32_t i = threadIdx.x; i < n_bins; i += 256u) cnt[i] = 0u;
    __syncthreads();
    auto lds_add = [&](uint32_t, uint32_t b, uint32_t len) { (void)__hip_atomic_fetch_add(&cnt[b], len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    uint32_t r_u, r_b, r_len;
    dh_walk<false>(depth, g_base, n, 0u, n, ends_p, n_unitigs, total_len, k, n_bins, bin_width, r_u, r_b, r_len, lds_add);
    uint32_t u0 = 0, b0 = 0;
    if (dh_uniform<false>(r_u, r_b, r_len, &u0, &b0)) {   // the hot bin: one add for the wave
        const uint32_t tot = fin_wave_sum(r_len);
        if ((threadIdx.x & 63u) == 0u) lds_add(0u, b0, tot);
    } else if (r_len != 0u) lds_add(0u, r_b, r_len);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_bins; i += 256u) dh_add64(hist + i, cnt[i]);
}

// V: uint32[(u_hi - u_lo) * n_bins], zeroed by the launcher; [lo, hi): the window of the stage that holds what this chunk has of the unitigs [u_lo, u_hi)
__global__ __launch_bounds__(256) void fin_dh_unitig_kernel(const uint32_t* depth, uint64_t g_base, uint64_t n, uint64_t lo, uint64_t hi, const uint32_t* ends_p,
                                                            uint32_t n_unitigs, uint64_t total_len, uint32_t k, uint32_t n_bins, uint32_t bin_width, uint32_t u_lo,
                                                            uint32_t u_hi, uint32_t* V) {
    auto add = [&](uint32_t u, uint32_t b, uint32_t len) {   // (b < n_bins always; a unitig outside the sub-range has no row)
        if (u >= u_lo && u < u_hi) (void)__hip_atomic_fetch_add(V + (uint64_t)(u - u_lo) * n_bins + b, len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    uint32_t r_u, r_b, r_len;
    dh_walk<true>(depth, g_base, n, lo, hi, ends_p, n_unitigs, total_len, k, n_bins, bin_width, r_u, r_b, r_len, add);
    uint32_t u0 = 0, b0 = 0;
    if (dh_uniform<true>(r_u, r_b, r_len, &u0, &b0)) {
        const uint32_t tot = fin_wave_sum(r_len);
        if ((threadIdx.x & 63u) == 0u) add(u0, b0, tot);
    } else if (r_len != 0u) add(r_u, r_b, r_len);
}

// block x: word group x % n_groups (words 4 g + wave), bin slice (x / n_groups) % n_slices (bins [16 s, 16 s + 16)), chunk x / n_groups / n_slices (unitigs
// [u_lo + chunk * c, ...) below u_hi); chunk is a multiple of 64.  out: uint64[n_colors][2][n_bins]
__global__ __launch_bounds__(256) void fin_dh_project_kernel(const ull* bits, uint32_t W, uint32_t n_groups, uint32_t n_slices, uint32_t u_lo, uint32_t u_hi, uint32_t chunk,
                                                             uint32_t n_colors, const uint8_t* cls, const uint32_t* V, uint32_t n_bins, ull* out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (blockIdx.x % n_groups) * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= W) return;   // wave-uniform
    const uint32_t rest = blockIdx.x / n_groups;
    const uint32_t b0 = (rest % n_slices) * FIN_DH_S, nb = std::min(FIN_DH_S, n_bins - b0);
    const uint64_t c0 = (uint64_t)u_lo + (uint64_t)(rest / n_slices) * chunk;
    const uint32_t c1 = (uint32_t)std::min<uint64_t>(u_hi, c0 + chunk);
    uint32_t all[FIN_DH_S], only[FIN_DH_S];
#pragma unroll
    for (uint32_t i = 0; i < FIN_DH_S; i++) { all[i] = 0u; only[i] = 0u; }
    for (uint64_t base = c0; base < c1; base += 64u) {   // wave-uniform
        const uint64_t u = base + lane;
        const ull word = u < c1 ? bits[u * W + w] : 0ull;
        ull live = __ballot(word != 0ull);
        if (live == 0ull) continue;
        const uint32_t c = word != 0ull ? cls[u] : 0u;
        for (; live; live &= live - 1ull) {
            const int src = __ffsll((long long)live) - 1;
            const ull wd = fin_bcast64(word, src);
            const bool one = fin_bcast(c, src) == 1u;
            const uint32_t* const row = V + (base + (uint32_t)src - u_lo) * n_bins + b0;   // wave-uniform
            const bool mine = (wd >> lane) & 1ull;
#pragma unroll
            for (uint32_t i = 0; i < FIN_DH_S; i++) {
                const uint32_t v = i < nb ? row[i] : 0u;
                if (mine) { all[i] += v; if (one) only[i] += v; }
            }
        }
    }
    const uint32_t color = 64u * w + lane;
    if (color >= n_colors) return;   // (such a lane has added nothing: the bit cannot be set)
    ull* const o = out + (uint64_t)color * 2u * n_bins + b0;
#pragma unroll
    for (uint32_t i = 0; i < FIN_DH_S; i++)
        if (i < nb) { dh_add64(o + i, all[i]); dh_add64(o + n_bins + i, only[i]); }
}

// block x: bins [256 (x % n_bblk), ...), chunk x / n_bblk of the sub-range's unitigs
__global__ __launch_bounds__(256) void fin_dh_none_kernel(const uint8_t* cls, const uint32_t* V, uint32_t u_lo, uint32_t u_hi, uint32_t chunk, uint32_t n_bins, uint32_t n_bblk,
                                                          ull* none) {
    const uint32_t b = (blockIdx.x % n_bblk) * 256u + threadIdx.x;
    const uint64_t c0 = (uint64_t)u_lo + (uint64_t)(blockIdx.x / n_bblk) * chunk;
    const uint32_t c1 = (uint32_t)std::min<uint64_t>(u_hi, c0 + chunk);
    if (b >= n_bins) return;
    uint32_t acc = 0;
    for (uint64_t u = c0; u < c1; u++)
        if (cls[u] == 0u) acc += V[(u - u_lo) * n_bins + b];
    dh_add64(none + b, acc);
}

extern "C" uint32_t fin_depthhist_max_bins(void) { return FIN_DH_MAX_BINS; }

// hist[n_bins] (uint64, zeroed by the caller before the first chunk) += the spectrum of depth[0 .. n), the depths of text positions g_base .. g_base + n (all below
// total_len); depth is 16-byte aligned
extern "C" int fin_launch_depth_spectrum(const uint32_t* depth, uint64_t g_base, uint64_t n, const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len, uint32_t k,
                                         uint32_t n_bins, uint32_t bin_width, uint64_t* hist, hipStream_t stream) {
    if (n_bins == 0 || n_bins > FIN_DH_MAX_BINS || bin_width == 0 || g_base + n > total_len) return (int)hipErrorInvalidValue;
    if (n == 0 || n_unitigs == 0) return 0;
    const uint64_t lanes = (n + FIN_DH_P - 1u) / FIN_DH_P;
    hipLaunchKernelGGL(fin_dh_spectrum_kernel, dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, stream, depth, g_base, n, ends_p, n_unitigs, total_len, k, n_bins,
                       bin_width, (ull*)hist);
    return (int)hipGetLastError();
}

// one sub-range of unitigs [u_lo, u_hi) of one staged chunk: V (uint32[(u_hi - u_lo) * n_bins]) is zeroed, binned from the window [lo, hi) of the stage and
// projected -- out uint64[n_colors][2][n_bins] and none uint64[n_bins] are ADDED to (the caller zeroes them before the first sub-range).  cls: the class byte of every
// unitig (fin_launch_color_classes).  variant: 0, lane = colour (the only one built)
extern "C" int fin_launch_color_depth_hist(const uint32_t* depth, uint64_t g_base, uint64_t n, uint64_t lo, uint64_t hi, const uint32_t* ends_p, uint32_t n_unitigs,
                                           uint64_t total_len, uint32_t k, uint32_t n_bins, uint32_t bin_width, uint32_t u_lo, uint32_t u_hi, uint32_t* V, const void* bits,
                                           uint32_t W, uint32_t n_colors, const void* cls, uint32_t variant, uint64_t* out, uint64_t* none, hipStream_t stream) {
    if (n_bins == 0 || n_bins > FIN_DH_MAX_BINS || bin_width == 0 || g_base + n > total_len || lo > hi || hi > n || hi - lo >= (1ull << 32) || u_lo > u_hi || u_hi > n_unitigs ||
        W == 0 || W > 64u || n_colors == 0 || n_colors > 64u * W || n_colors + 64u <= 64u * W || n_unitigs >= 0x80000000u || variant != 0u)
        return (int)hipErrorInvalidValue;
    if (lo == hi || u_lo == u_hi) return 0;
    const uint32_t n_sub = u_hi - u_lo;
    hipError_t e = hipMemsetAsync(V, 0, (size_t)n_sub * n_bins * 4u, stream);
    if (e != hipSuccess) return (int)e;
    const uint64_t lanes = (hi + FIN_DH_P - 1u) / FIN_DH_P - lo / FIN_DH_P;
    hipLaunchKernelGGL(fin_dh_unitig_kernel, dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, stream, depth, g_base, n, lo, hi, ends_p, n_unitigs, total_len, k, n_bins,
                       bin_width, u_lo, u_hi, V);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    // unitigs per wave of the projection: about 2048 blocks in all, never under 64 unitigs
    const uint32_t n_groups = (W + 3u) / 4u, n_slices = (n_bins + FIN_DH_S - 1u) / FIN_DH_S;
    const uint32_t chunks = std::max(1u, 2048u / (n_groups * n_slices));
    const uint32_t chunk = (std::max(64u, (n_sub + chunks - 1u) / chunks) + 63u) / 64u * 64u;
    const uint32_t n_chunks = (n_sub + chunk - 1u) / chunk;
    hipLaunchKernelGGL(fin_dh_project_kernel, dim3(n_chunks * n_groups * n_slices), dim3(256), 0, stream, (const ull*)bits, W, n_groups, n_slices, u_lo, u_hi, chunk, n_colors,
                       (const uint8_t*)cls, (const uint32_t*)V, n_bins, (ull*)out);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const uint32_t n_bblk = (n_bins + 255u) / 256u, nchunk = (std::max(256u, (n_sub + 255u) / 256u) + 63u) / 64u * 64u;
    hipLaunchKernelGGL(fin_dh_none_kernel, dim3(((n_sub + nchunk - 1u) / nchunk) * n_bblk), dim3(256), 0, stream, (const uint8_t*)cls, (const uint32_t*)V, u_lo, u_hi, nchunk,
                       n_bins, n_bblk, (ull*)none);
    return (int)hipGetLastError();
}
