// fin_bootstrap.hip -- BOOTSTRAP REPLICATES of the abundance estimate: each replicate's class counts drawn on the device over the dense class list of a
// fin_eqclasses (include/finito_amd.h: fin_eqclasses_bootstrap).  The list lies in HBM as fin_abundance.hip takes it: rows uint64[C][W] and
// reads uint64[C]; a replicate's counts go where the reads went in fin_launch_ab_iteration, which runs unchanged.
//
// A POISSON BOOTSTRAP KEYED BY THE CLASS'S ROW.  Every read of every class gets an independent multiplicity X with the Poisson(1) distribution quantised to
// 2^-32 (at most 13), from Philox4x32-10 under key = seed and counter = {the row's 64-bit hash h_j, the read's block i inside the class, the replicate b}
// (fin_bootrng.h); n_j^(b) = the sum of X over the class's n_j reads, N_b = the sum of n_j^(b).  Exact integers, a function of (row, n_j, seed, b) alone: the
// dense list's order -- the table's slot order, which depends on claim races -- does not enter, and neither does which wave runs first.
//
// INTEGER ADDS ONLY, and NO LANE WAITS FOR ANOTHER LANE'S STORE: kernel boundaries are the only synchronisation between launches, __syncthreads the only one
// inside.  Every loop bound is a kernel argument or a constant.
//   once per call   fin_boot_rowhash_kernel   h[C]: W = 1 a lane per class; W > 1 a wave per class, lane i word i, an xor over the wave (fin_ec_claim_kernel's).
//                   fin_boot_slabs_kernel     slabs[j] = ceil(n_j / 4096) as uint32 (n_j < 2^40); fin_launch_blk_scan makes their exclusive prefix and total S.
//   per replicate   fin_boot_resample_kernel  counts[C] and the N_b word zeroed before it.  One wave per slab s < S (a launch has at most 2^20 blocks: the waves stride over
//                                             the slabs behind 2^22, the bound S a kernel argument): a wave-uniform binary search in the prefix
//                                             (bound: C) finds the class j, slab t = s - prefix[j] holds the reads [4096 t, min(n_j, 4096 (t + 1))) -- the
//                                             Philox blocks 1024 t + l + 64 m of lane l, m < 16.  The lane sums X over the words of reads below n_j, a butterfly
//                                             sums the wave, lane 0 adds to counts[j] (a plain store where the class is one slab); the block's four waves are
//                                             summed through LDS and thread 0 adds to N_b.
#include <algorithm>

#include "fin_bootrng.h"
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_wave.h"

#define FIN_BOOT_BLK 256u
#define FIN_BOOT_MAX_GRID (1u << 20)   // blocks of a resample launch: gridDim.x * blockDim.x stays below 2^32

namespace {
typedef unsigned long long ull;
}

__global__ __launch_bounds__(256) void fin_boot_rowhash_kernel(const ull* rows, uint64_t C, uint32_t W, ull* h) {
    const uint32_t lane = threadIdx.x & 63u;
    if (W == 1u) {
        const uint64_t j = (uint64_t)blockIdx.x * FIN_BOOT_BLK + threadIdx.x;
        if (j < C) h[j] = ec_word_hash(rows[j], 0u);
    } else {
        const uint64_t j = (uint64_t)blockIdx.x * (FIN_BOOT_BLK / 64u) + (threadIdx.x >> 6);   // wave-uniform
        if (j >= C) return;
        const uint64_t v = ec_wave_xor(lane < W ? ec_word_hash(rows[j * W + lane], lane) : 0ull);
        if (lane == 0u) h[j] = v;
    }
}

__global__ __launch_bounds__(256) void fin_boot_slabs_kernel(const ull* reads, uint64_t C, uint32_t* slabs) {
    const uint64_t j = (uint64_t)blockIdx.x * FIN_BOOT_BLK + threadIdx.x;
    if (j < C) slabs[j] = (uint32_t)((reads[j] + (FIN_BOOT_SLAB - 1u)) / FIN_BOOT_SLAB);
}

// prefix[j]: the slabs of the classes before j (exclusive, ascending); S: their total
__global__ __launch_bounds__(256) void fin_boot_resample_kernel(const ull* h, const ull* reads, const uint64_t* prefix, uint64_t C, uint64_t S, uint64_t seed, uint32_t b,
                                                                ull* counts, ull* n_b) {
    __shared__ ull lds_w[FIN_BOOT_BLK / 64u];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    ull wave_tot = 0;                       // (kept in every lane, used by lane 0)
    for (uint64_t s = (uint64_t)blockIdx.x * (FIN_BOOT_BLK / 64u) + wave; s < S; s += (uint64_t)gridDim.x * (FIN_BOOT_BLK / 64u)) {   // wave-uniform
        uint64_t lo = 0, hi = C;            // the last j in [0, C) with prefix[j] <= s (prefix[0] = 0): at most 26 steps, C <= 2^26
        while (hi - lo > 1ull) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (prefix[mid] <= s) lo = mid; else hi = mid;
        }
        const uint64_t j = lo, t = s - prefix[j], n = reads[j], hj = h[j];
        const uint64_t i0 = t * (FIN_BOOT_SLAB / 4u), n_blocks = (n + 3ull) >> 2;   // the class's Philox blocks: [0, n_blocks)
        if (i0 >= n_blocks) continue;       // (never, for a prefix made from these reads: a hand-made one is not trusted)
        const uint32_t here = (uint32_t)min((uint64_t)(FIN_BOOT_SLAB / 4u), n_blocks - i0);
        uint32_t sum = 0;
        for (uint32_t m = 0; m < FIN_BOOT_SLAB / 256u; m++) {
            const uint32_t k = lane + 64u * m;
            if (k < here) sum += fin_boot_block_sum(hj, i0 + k, n, b, seed);
        }
        sum = fin_wave_sum(sum);
        wave_tot += sum;
        if (lane == 0u) {
            if (n <= FIN_BOOT_SLAB) counts[j] = (ull)sum;
            else if (sum) (void)atomicAdd(counts + j, (ull)sum);
        }
    }
    if (lane == 0u) lds_w[wave] = wave_tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        const ull tot = lds_w[0] + lds_w[1] + lds_w[2] + lds_w[3];
        if (tot) (void)atomicAdd(n_b, tot);
    }
}

// h[C] from rows[C][W]
extern "C" int fin_launch_ab_rowhash(const void* rows, uint64_t C, uint32_t W, void* h, hipStream_t stream) {
    if (C == 0 || C > (1ull << 26) || W == 0 || W > 64u) return (int)hipErrorInvalidValue;
    const uint64_t per = W == 1u ? FIN_BOOT_BLK : FIN_BOOT_BLK / 64u;
    hipLaunchKernelGGL(fin_boot_rowhash_kernel, dim3((uint32_t)((C + per - 1u) / per)), dim3(FIN_BOOT_BLK), 0, stream, (const ull*)rows, C, W, (ull*)h);
    return (int)hipGetLastError();
}
// slabs[C] (uint32), their exclusive prefix[C] and *total from reads[C] (each below 2^40)
extern "C" int fin_launch_ab_slabs(const void* reads, uint64_t C, uint32_t* slabs, uint64_t* prefix, uint64_t* total, hipStream_t stream) {
    if (C == 0 || C > (1ull << 26)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fin_boot_slabs_kernel, dim3((uint32_t)((C + FIN_BOOT_BLK - 1u) / FIN_BOOT_BLK)), dim3(FIN_BOOT_BLK), 0, stream, (const ull*)reads, C, slabs);
    return fin_launch_blk_scan(slabs, (uint32_t)C, prefix, total, stream);
}
// replicate b: counts[C] and *n_b, both zeroed by the caller before the launch.  S: the total of fin_launch_ab_slabs, read back by the host
extern "C" int fin_launch_ab_resample(const void* h, const void* reads, const uint64_t* prefix, uint64_t C, uint64_t S, uint64_t seed, uint32_t b, void* counts, void* n_b,
                                      hipStream_t stream) {
    if (C == 0 || C > (1ull << 26) || b >= FIN_BOOT_MAX || S > (1ull << 33)) return (int)hipErrorInvalidValue;
    if (S == 0) return 0;
    const uint64_t nb = std::min<uint64_t>((S + FIN_BOOT_BLK / 64u - 1u) / (FIN_BOOT_BLK / 64u), FIN_BOOT_MAX_GRID);   // (the waves stride over the slabs behind that)
    hipLaunchKernelGGL(fin_boot_resample_kernel, dim3((uint32_t)nb), dim3(FIN_BOOT_BLK), 0, stream, (const ull*)h, (const ull*)reads, prefix, C, S, seed, b, (ull*)counts,
                       (ull*)n_b);
    return (int)hipGetLastError();
}
