// fin_assign.hip -- READS ASSIGNED TO REFERENCES from per-colour weights: which colours of a read's (or a fragment's) row the read belongs to, once the
// references' abundances are known (include/finito_amd.h: fin_assign_rows).  Rows R_r uint64[n][W] in HBM, weights x[c] and thresholds thr[c], IEEE
// double throughout:
//   s_w = x over the set bits of word w, ascending from 0.0      d = the s_w folded in halves over wp2 (fin_absum.h: fin_ab_denoms_kernel's d_j, bit for bit)
//   c is ASSIGNED iff bit c of R_r, x[c] > 0, d > 0 and x[c] >= thr[c] * d (one multiply, one compare)
//   best = the colour of the row with the largest x[c], the smaller colour on a tie; FIN_NO_COLOR unless d > 0
// Out, per row: the assigned row A_r (a subset of R_r) and the head {n_assigned, best}.  Per accumulator, exact integers: assigned[c] (rows with c in A_r),
// sole[c] (rows whose A_r is {c}) and the counters {rows, unaligned, unassigned, multi}.
//
// NO FLOATING-POINT ATOMICS; NO LANE WAITS FOR ANOTHER LANE'S STORE; every output word of a row has one writer; every loop bound is a kernel argument.
//   fin_assign_rows_kernel    block b owns the rows [b rpb, (b + 1) rpb).  x[] staged in LDS (8 bytes per colour), beside the block's two histograms uint32[64 W]
//                             (assigned, sole): 16 bytes per colour, 64 KB at 4096 colours -- two blocks per CU.  thr is NOT staged: a third 32 KB would leave one
//                             block per CU, and it is read only for a set bit with x > 0 of a row with d > 0, from a table of at most 32 KB that stays in L2.
//                             W = 1: a lane per row; the per-colour counts are ballots (lane c keeps colour c's), one LDS add per lane and wave at the end.
//                             W > 1: a wave per row, lane i word i (fin_col_pseudo_kernel's coalesced row load); d by the butterfly over wp2 lanes; best by a wave
//                             arg-max; the lane that owns a word stores its assigned word and adds its bits to the histograms; n_assigned is a wave sum.
//                             At the block's end the non-zero histogram entries go out as 64-bit global atomics, the counters as four per wave: no global atomic
//                             per row.
//   fin_assign_column_kernel  bit c of every assigned row as a bitmap uint64[(n + 63) / 64], a word per ballot, and the count per block of 256 rows: the layout
//                             fin_launch_blk_scan and fin_launch_screen_ids (fin_readsum.hip) turn into the ascending list of the rows that have colour c.
#include <algorithm>

#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_wave.h"
#include "fin_absum.h"

#define FIN_ASG_BLK 256u
#define FIN_ASG_NO_COLOR 0xFFFFFFFFu

namespace {
typedef unsigned long long ull;

// a lane's word of a row: its assigned bits, and the word's best colour (bx < 0: the word is empty).  xs / ts: the word's 64 weights (LDS) and thresholds
__device__ __forceinline__ ull asg_word(ull word, const double* xs, const double* ts, double d, uint32_t c0, double& bx, uint32_t& bc) {
    ull a = 0ull;
    bx = -1.0; bc = FIN_ASG_NO_COLOR;
    for (ull m = word; m; m &= m - 1ull) {   // ascending: the first of equal weights stays
        const uint32_t b = (uint32_t)__ffsll((long long)m) - 1u;
        const double v = xs[b];
        if (v > bx) { bx = v; bc = c0 + b; }
        if (v > 0.0 && d > 0.0 && v >= ts[b] * d) a |= 1ull << b;
    }
    return a;
}
}  // namespace

// rows [blockIdx.x rpb, ...) of n.  x, thr: 64 W doubles (0 behind n_colors); last_mask: the colours of word W - 1.  out_rows, heads: may be null
__global__ __launch_bounds__(256) void fin_assign_rows_kernel(const ull* rows, uint64_t n, uint32_t W, uint32_t wp2, uint32_t n_colors, ull last_mask, uint32_t rpb,
                                                              const double* x, const double* thr, ull* out_rows, uint2* heads, ull* assigned, ull* sole, ull* counters) {
    extern __shared__ double lds_x[];       // 64 W doubles, then hist_a and hist_s: 64 W uint32 each
    uint32_t* const hist_a = (uint32_t*)(lds_x + 64u * W);
    uint32_t* const hist_s = hist_a + 64u * W;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < 64u * W; i += FIN_ASG_BLK) { lds_x[i] = x[i]; hist_a[i] = 0u; hist_s[i] = 0u; }
    __syncthreads();
    const uint64_t r0 = (uint64_t)blockIdx.x * rpb, r1 = min(n, r0 + rpb);
    uint32_t n_rows = 0, n_unal = 0, n_unas = 0, n_multi = 0;   // wave-uniform
    if (W == 1u) {
        uint32_t acc_a = 0, acc_s = 0;      // lane c: colour c's counts over the wave's rows
        for (uint64_t base = r0 + 64u * wave; base < r1; base += FIN_ASG_BLK) {   // wave-uniform
            const uint64_t r = base + lane;
            const bool in = r < r1;
            const ull word = in ? rows[r] & last_mask : 0ull;
            const double d = ab_bits_sum(word, lds_x);
            double bx; uint32_t bc;
            const ull a = asg_word(word, lds_x, thr, d, 0u, bx, bc);
            const uint32_t na = (uint32_t)__popcll(a);
            if (in) {
                if (out_rows) out_rows[r] = a;
                if (heads) heads[r] = make_uint2(na, d > 0.0 ? bc : FIN_ASG_NO_COLOR);
            }
            for (uint32_t c = 0; c < n_colors; c++) {
                const bool has = (a >> c) & 1ull;
                const uint32_t ca = (uint32_t)__popcll(__ballot(has)), cs = (uint32_t)__popcll(__ballot(has && na == 1u));
                if (lane == c) { acc_a += ca; acc_s += cs; }
            }
            n_rows += (uint32_t)__popcll(__ballot(in));
            n_unal += (uint32_t)__popcll(__ballot(in && word == 0ull));
            n_unas += (uint32_t)__popcll(__ballot(word != 0ull && a == 0ull));
            n_multi += (uint32_t)__popcll(__ballot(na >= 2u));
        }
        if (acc_a) atomicAdd(&hist_a[lane], acc_a);   // (lane < n_colors)
        if (acc_s) atomicAdd(&hist_s[lane], acc_s);
    } else {
        const uint32_t wl = min(lane, W - 1u);
        const double* const xs = lds_x + 64u * wl;
        const double* const ts = thr + 64u * wl;
        for (uint64_t r = r0 + wave; r < r1; r += FIN_ASG_BLK / 64u) {   // wave-uniform
            ull word = lane < W ? rows[r * W + lane] : 0ull;
            if (lane == W - 1u) word &= last_mask;
            const double d = ab_butterfly(ab_bits_sum(word, xs), wp2);   // (lanes behind W: 0.0; the same in every lane below wp2)
            double bx; uint32_t bc;
            const ull a = asg_word(word, xs, ts, d, 64u * wl, bx, bc);
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {   // the wave's arg-max; a lane without a set bit holds (-1, no colour)
                const double ox = __shfl_xor(bx, s);
                const uint32_t oc = (uint32_t)__shfl_xor((int)bc, s);
                if (ox > bx || (ox == bx && oc < bc)) { bx = ox; bc = oc; }
            }
            const uint32_t na = fin_wave_sum((uint32_t)__popcll(a));
            if (out_rows && lane < W) out_rows[r * W + lane] = a;
            if (heads && lane == 0u) heads[r] = make_uint2(na, d > 0.0 ? bc : FIN_ASG_NO_COLOR);
            for (ull m = a; m; m &= m - 1ull) {
                const uint32_t c = 64u * wl + (uint32_t)__ffsll((long long)m) - 1u;
                atomicAdd(&hist_a[c], 1u);
                if (na == 1u) atomicAdd(&hist_s[c], 1u);
            }
            const bool empty = __ballot(word != 0ull) == 0ull;
            n_rows++;
            if (empty) n_unal++;
            else if (na == 0u) n_unas++;
            if (na >= 2u) n_multi++;
        }
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < n_colors; c += FIN_ASG_BLK) {
        const uint32_t va = hist_a[c], vs = hist_s[c];
        if (va) atomicAdd(&assigned[c], (ull)va);
        if (vs) atomicAdd(&sole[c], (ull)vs);
    }
    if (lane == 0u) {
        if (n_rows) atomicAdd(&counters[0], (ull)n_rows);
        if (n_unal) atomicAdd(&counters[1], (ull)n_unal);
        if (n_unas) atomicAdd(&counters[2], (ull)n_unas);
        if (n_multi) atomicAdd(&counters[3], (ull)n_multi);
    }
}

// bits[w] = the ballot of "row 64 w + lane has colour c assigned"; blk_sum[block] = how many of the block's 256 rows have.  A lane beyond n has not
__global__ __launch_bounds__(256) void fin_assign_column_kernel(const ull* arows, uint32_t n, uint32_t W, uint32_t c, ull* bits, uint32_t* blk_sum) {
    __shared__ uint32_t lds_w[4];
    const uint32_t r = blockIdx.x * FIN_ASG_BLK + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool has = r < n && ((arows[(uint64_t)r * W + (c >> 6)] >> (c & 63u)) & 1ull);
    const ull w = __ballot(has);
    const uint32_t word = blockIdx.x * 4u + wave;
    if (lane == 0u) {
        if (word < (n + 63u) / 64u) bits[word] = w;
        lds_w[wave] = (uint32_t)__popcll(w);
    }
    __syncthreads();
    if (threadIdx.x == 0) blk_sum[blockIdx.x] = lds_w[0] + lds_w[1] + lds_w[2] + lds_w[3];
}

// rows per block: option "assign_rpb", or (0) 1024 and more once that would make over 2048 blocks; never so few that there would be over 2^20 blocks
extern "C" uint32_t fin_assign_rpb(uint64_t n_rows, uint32_t assign_rpb) {
    uint64_t rpb = assign_rpb;
    if (rpb == 0) rpb = std::max<uint64_t>(1024u, ((n_rows + 2047u) / 2048u + 255u) / 256u * 256u);
    return (uint32_t)std::max<uint64_t>(rpb, (n_rows + (1u << 20) - 1u) >> 20);
}
extern "C" int fin_launch_assign_rows(const void* rows, uint64_t n_rows, uint32_t W, uint32_t n_colors, uint32_t assign_rpb, const double* x, const double* thr,
                                      void* out_rows, void* heads, uint64_t* assigned, uint64_t* sole, uint64_t* counters, hipStream_t stream) {
    if (W == 0 || W > 64u || n_colors == 0 || n_colors > 64u * W || n_colors + 64u <= 64u * W || n_rows > 0xFFFFFFFFull) return (int)hipErrorInvalidValue;
    if (n_rows == 0) return 0;
    uint32_t wp2 = 1;
    while (wp2 < W) wp2 <<= 1;
    const ull last_mask = (n_colors & 63u) ? (1ull << (n_colors & 63u)) - 1ull : ~0ull;
    const uint32_t rpb = fin_assign_rpb(n_rows, assign_rpb);
    hipLaunchKernelGGL(fin_assign_rows_kernel, dim3((uint32_t)((n_rows + rpb - 1u) / rpb)), dim3(FIN_ASG_BLK), (size_t)W * 1024u, stream, (const ull*)rows, n_rows, W, wp2,
                       n_colors, last_mask, rpb, x, thr, (ull*)out_rows, (uint2*)heads, (ull*)assigned, (ull*)sole, (ull*)counters);
    return (int)hipGetLastError();
}
extern "C" int fin_launch_assign_column(const void* arows, uint32_t n_rows, uint32_t W, uint32_t color, uint64_t* bits, uint32_t* blk_sum, uint64_t* blk_off,
                                        uint64_t* total, hipStream_t stream) {
    const uint32_t nb = fin_rsm_blocks(n_rows);
    if (nb == 0) return (int)hipMemsetAsync(total, 0, 8, stream);
    if (W == 0 || color >= 64u * W) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fin_assign_column_kernel, dim3(nb), dim3(FIN_ASG_BLK), 0, stream, (const ull*)arows, n_rows, W, color, (ull*)bits, blk_sum);
    return fin_launch_blk_scan(blk_sum, nb, blk_off, total, stream);
}
