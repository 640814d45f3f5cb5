// fin_abundance.hip -- ABUNDANCES from the equivalence classes: EM over the dense class list of a fin_eqclasses (include/finito_amd.h:
// fin_eqclasses_abundance).  The classes (R_j, n_j), j < C, lie in HBM as the download's gather leaves them: rows uint64[C][W] and reads
// uint64[C].  One iteration t, all in IEEE double:
//   x_c = alpha_c / len[c]      d_j = sum of x_c over c in R_j      ll_t = sum of n_j log(d_j / N)      q_j = n_j / d_j
//   S_c = sum of q_j over the classes that contain c                  alpha'_c = x_c S_c
// and it has converged when |alpha'_c - alpha_c| <= tol max(alpha'_c, 1) for every colour.
//
// NO FLOATING-POINT ATOMICS, and no sum whose order depends on which wave runs first: every sum below has a fixed order that is a function of C, W and
// `chunk` alone, so two estimates over the same dense list are bit-identical.  NO LANE WAITS FOR ANOTHER LANE'S STORE: an iteration is four launches on one
// stream and the kernel boundaries are the only synchronisation.  Every loop bound is a kernel argument.
//   1  fin_ab_denoms_kernel   x[] staged in LDS (8 bytes per colour: 32 KB at 4096 colours).  Block b owns the classes [b cpb, (b + 1) cpb).  W = 1: a lane per
//                             class.  W > 1: a wave per class, lane i word i (fin_col_pseudo_kernel's coalesced row load), the lane adds x over its word's set
//                             bits in ascending order, a butterfly over the lanes gives d_j.  q_j is stored, the wave's n_j log(d_j / N) are summed in class
//                             order, the block's four waves in wave order: ll_part[b].
//   2  fin_ab_colsum_kernel   a wave per (chunk of `chunk` classes, word w), lane b owns colour 64 w + b and one accumulator.  Per step the wave loads word w and
//                             q of 64 consecutive classes from the WORD-MAJOR copy rowsT[W][C] (coalesced), takes a ballot of the non-zero words and walks those
//                             in ascending order with readlane: lane b adds q where bit b is set -- fin_col_pseudo_kernel's count loop.  part[chunk][64 w + b].
//   3  fin_ab_colred_kernel   a block of 16 waves per word w: wave v sums its sixteenth of the chunks in ascending order, lane b colour 64 w + b; the sixteen
//                             are summed in wave order: S_c.  alpha' = x S, the change test, next x; blk_ok[w] and blk_chg[w].  (One block for all colours
//                             would read up to 32 MB of partials through one CU: this is why the update is two launches.)
//   4  fin_ab_finish_kernel   one wave: ll_t from ll_part (lane l its share in ascending order, then a butterfly), the AND of blk_ok and the max of blk_chg
//                             (both order-free); trace[t], and the state word {done, iters}.
// The kernels of an iteration return at once when `done` is set (it is only ever written by kernel 4, a launch earlier), so iterations enqueued behind the
// criterion change nothing; the host enqueues groups of iterations and reads the 8 bytes between groups.
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_wave.h"
#include "fin_absum.h"

#define FIN_AB_BLK 256u
#define FIN_AB_RED_WAVES 16u

namespace {
typedef unsigned long long ull;
}  // namespace

// rowsT[w][j] = rows[j][w]: a tile of 64 classes through LDS, both sides coalesced
__global__ __launch_bounds__(256) void fin_ab_transpose_kernel(const ull* rows, uint64_t C, uint32_t W, ull* rowsT) {
    __shared__ ull tile[64][65];
    const uint64_t base = (uint64_t)blockIdx.x * 64u;
    const uint32_t n_here = (uint32_t)min((uint64_t)64u, C - base);
    for (uint32_t i = threadIdx.x; i < n_here * W; i += 256u) tile[i / W][i % W] = rows[base * W + i];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 64u * W; i += 256u) {
        const uint32_t w = i >> 6, j = i & 63u;
        if (j < n_here) rowsT[(uint64_t)w * C + base + j] = tile[j][w];
    }
}

// pass 1.  cpb: classes per block, a multiple of 256; wp2: the power of two >= W; x: 64 W doubles (0 behind n_colors)
__global__ __launch_bounds__(256) void fin_ab_denoms_kernel(const FinAbState* st, const ull* rows, const ull* reads, uint64_t C, uint32_t W, uint32_t wp2, uint32_t cpb,
                                                            const double* x, double n_total, double* q, double* ll_part) {
    extern __shared__ double lds_x[];       // 64 W doubles, then 4 for the waves' sums
    if (st->done) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < 64u * W; i += FIN_AB_BLK) lds_x[i] = x[i];
    __syncthreads();
    const uint64_t j0 = (uint64_t)blockIdx.x * cpb, j1 = min(C, j0 + cpb);
    double ll = 0.0;
    if (W == 1u) {
        for (uint64_t j = j0 + threadIdx.x; j < j1; j += FIN_AB_BLK) {
            const double d = ab_bits_sum(rows[j], lds_x), n = (double)reads[j];
            q[j] = d > 0.0 ? n / d : 0.0;
            if (d > 0.0) ll += n * log(d / n_total);
        }
        ll = ab_butterfly(ll, 64u);
    } else {
        for (uint64_t j = j0 + wave; j < j1; j += FIN_AB_BLK / 64u) {   // wave-uniform
            const ull word = lane < W ? rows[j * W + lane] : 0ull;
            const double d = ab_butterfly(ab_bits_sum(word, lds_x + 64u * min(lane, W - 1u)), wp2);   // (lanes behind W: 0.0)
            if (lane == 0u) {
                const double n = (double)reads[j];
                q[j] = d > 0.0 ? n / d : 0.0;
                if (d > 0.0) ll += n * log(d / n_total);
            }
        }
    }
    double* const lds_w = lds_x + 64u * W;
    if (lane == 0u) lds_w[wave] = ll;
    __syncthreads();
    if (threadIdx.x == 0) ll_part[blockIdx.x] = ((lds_w[0] + lds_w[1]) + lds_w[2]) + lds_w[3];
}

// pass 2.  grid (ceil(n_chunks / 4), W): wave g of the launch takes chunk g
__global__ __launch_bounds__(256) void fin_ab_colsum_kernel(const FinAbState* st, const ull* rowsT, const double* q, uint64_t C, uint32_t W, uint32_t chunk,
                                                            uint32_t n_chunks, double* part) {
    if (st->done) return;
    const uint32_t lane = threadIdx.x & 63u, k = blockIdx.x * (FIN_AB_BLK / 64u) + (threadIdx.x >> 6), w = blockIdx.y;
    if (k >= n_chunks) return;              // wave-uniform
    const uint64_t j0 = (uint64_t)k * chunk, j1 = min(C, j0 + chunk);
    const ull* const col = rowsT + (uint64_t)w * C;
    double acc = 0.0;
    for (uint64_t j = j0; j < j1; j += 64u) {
        const bool in = j + lane < j1;
        const ull word = in ? col[j + lane] : 0ull;
        const ull qb = in ? (ull)__double_as_longlong(q[j + lane]) : 0ull;
        ull todo = __ballot(word != 0ull);
        while (todo) {                      // the classes of this step that have a colour of word w, ascending
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const ull m = fin_bcast64(word, src);
            const double qv = __longlong_as_double((long long)fin_bcast64(qb, src));
            if ((m >> lane) & 1ull) acc += qv;
        }
    }
    part[(uint64_t)k * (64u * W) + 64u * w + lane] = acc;
}

// pass 3.  grid W, 1024 threads: wave v sums the chunks [v per, (v + 1) per), per = ceil(n_chunks / 16)
__global__ __launch_bounds__(1024) void fin_ab_colred_kernel(const FinAbState* st, const double* part, uint32_t n_chunks, uint32_t W, uint32_t n_colors, const double* len,
                                                             double tol, double* alpha, double* x, uint32_t* blk_ok, double* blk_chg) {
    __shared__ double lds_s[FIN_AB_RED_WAVES][64];
    if (st->done) return;
    const uint32_t lane = threadIdx.x & 63u, v = threadIdx.x >> 6, w = blockIdx.x, c = 64u * w + lane;
    const uint32_t per = (n_chunks + FIN_AB_RED_WAVES - 1u) / FIN_AB_RED_WAVES;
    const uint32_t k0 = min(n_chunks, v * per), k1 = min(n_chunks, k0 + per);
    double s = 0.0;
#pragma unroll 8
    for (uint32_t k = k0; k < k1; k++) s += part[(uint64_t)k * (64u * W) + c];
    lds_s[v][lane] = s;
    __syncthreads();
    if (v != 0u) return;
    double S = lds_s[0][lane];
#pragma unroll
    for (uint32_t i = 1; i < FIN_AB_RED_WAVES; i++) S += lds_s[i][lane];
    bool ok = true;
    double chg = 0.0;
    if (c < n_colors) {
        const double a0 = alpha[c], a1 = x[c] * S;
        const double scale = a1 > 1.0 ? a1 : 1.0, diff = fabs(a1 - a0);
        ok = diff <= tol * scale;
        chg = diff / scale;
        alpha[c] = a1;
        x[c] = a1 / len[c];
    }
    chg = fin_wave_fmax(chg);
    const bool all_ok = __ballot(!ok) == 0ull;
    if (lane == 0u) { blk_ok[w] = all_ok ? 1u : 0u; blk_chg[w] = chg; }
}

// pass 4: one wave.  n_ll: the blocks of pass 1; t: the iteration
__global__ __launch_bounds__(64) void fin_ab_finish_kernel(FinAbState* st, const double* ll_part, uint32_t n_ll, const uint32_t* blk_ok, const double* blk_chg, uint32_t W,
                                                           uint32_t t, double* trace) {
    if (st->done) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t per = (n_ll + 63u) / 64u, b0 = min(n_ll, lane * per), b1 = min(n_ll, b0 + per);
    double ll = 0.0;
    for (uint32_t b = b0; b < b1; b++) ll += ll_part[b];
    ll = ab_butterfly(ll, 64u);
    const bool ok = lane < W ? blk_ok[lane] != 0u : true;   // W <= 64
    double chg = lane < W ? blk_chg[lane] : 0.0;
    chg = fin_wave_fmax(chg);
    const bool all_ok = __ballot(!ok) == 0ull;
    if (lane == 0u) {
        trace[t] = ll;
        st->loglik = ll; st->max_change = chg; st->iters = t + 1u;
        if (all_ok) st->done = 1u;
    }
}

// the geometry of one estimate, a function of C, W and option "ab_chunk" (0: auto) alone
extern "C" void fin_ab_geometry(uint64_t C, uint32_t W, uint32_t ab_chunk, uint32_t* cpb, uint32_t* n_ll, uint32_t* chunk, uint32_t* n_chunks) {
    const uint64_t per_blk = (C + 1023u) / 1024u;                         // at most 1024 blocks in pass 1 ...
    *cpb = (uint32_t)((per_blk + 255u) / 256u * 256u);
    if (*cpb == 0u) *cpb = 256u;
    *n_ll = (uint32_t)((C + *cpb - 1u) / *cpb);
    const uint64_t floor_chunk = ((C + 1023u) / 1024u + 63u) / 64u * 64u;   // ... and at most 1024 chunks in pass 2, whatever the option asks for
    uint64_t ch = ab_chunk ? (uint64_t)(ab_chunk + 63u) / 64u * 64u : 256u;
    if (ch < floor_chunk) ch = floor_chunk;
    *chunk = (uint32_t)ch;
    *n_chunks = (uint32_t)((C + ch - 1u) / ch);
}
// what an estimate over C classes needs beside rows and reads, in doubles: q[C] | part[n_chunks * 64 W] | ll_part[n_ll] | blk_chg[64]; and 64 u32 blk_ok
extern "C" int fin_launch_ab_transpose(const void* rows, uint64_t C, uint32_t W, void* rowsT, hipStream_t stream) {
    if (C == 0 || W == 0 || W > 64u) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fin_ab_transpose_kernel, dim3((uint32_t)((C + 63u) / 64u)), dim3(256), 0, stream, (const ull*)rows, C, W, (ull*)rowsT);
    return (int)hipGetLastError();
}
// iteration t of the estimate: four launches.  state: FinAbState (zeroed before iteration 0); rows[C][W] and rowsT[W][C] (the same array when W = 1); x, alpha,
// len: 64 W doubles each; trace: room for every t that is enqueued
extern "C" int fin_launch_ab_iteration(void* state, const void* rows, const void* rowsT, const void* reads, uint64_t C, uint32_t W, uint32_t n_colors, uint32_t ab_chunk,
                                       const double* len, double n_total, double tol, double* alpha, double* x, double* q, double* part, double* ll_part,
                                       uint32_t* blk_ok, double* blk_chg, uint32_t t, double* trace, hipStream_t stream) {
    if (C == 0 || C > (1ull << 26) || W == 0 || W > 64u || n_colors == 0 || n_colors > 64u * W) return (int)hipErrorInvalidValue;
    uint32_t cpb, n_ll, chunk, n_chunks, wp2 = 1;
    fin_ab_geometry(C, W, ab_chunk, &cpb, &n_ll, &chunk, &n_chunks);
    while (wp2 < W) wp2 <<= 1;
    FinAbState* const st = (FinAbState*)state;
    hipLaunchKernelGGL(fin_ab_denoms_kernel, dim3(n_ll), dim3(FIN_AB_BLK), (size_t)(64u * W + 4u) * 8, stream, st, (const ull*)rows, (const ull*)reads, C, W, wp2, cpb,
                       (const double*)x, n_total, q, ll_part);
    hipLaunchKernelGGL(fin_ab_colsum_kernel, dim3((n_chunks + 3u) / 4u, W), dim3(FIN_AB_BLK), 0, stream, st, (const ull*)rowsT, (const double*)q, C, W, chunk, n_chunks, part);
    hipLaunchKernelGGL(fin_ab_colred_kernel, dim3(W), dim3(64u * FIN_AB_RED_WAVES), 0, stream, st, (const double*)part, n_chunks, W, n_colors, len, tol, alpha, x, blk_ok,
                       blk_chg);
    hipLaunchKernelGGL(fin_ab_finish_kernel, dim3(1), dim3(64), 0, stream, st, (const double*)ll_part, n_ll, (const uint32_t*)blk_ok, (const double*)blk_chg, W, t, trace);
    return (int)hipGetLastError();
}
