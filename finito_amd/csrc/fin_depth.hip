// fin_depth.hip -- a run's per-position DEPTH over the unitig set: depth[g] = how many found pairs (u, off) had start(u) + off == g, for every position g of the
// concatenated unitig text (include/finito_amd.h: fin_depth, fin_batch_add_depth).  The third sibling: fin_hits.hip sums the depth over a unitig, fin_cover.hip
// says where it is above zero, this file keeps the depth itself.  The geometry is fin_cover's: start(u) = ends_p[u], total_len positions.
//
// The accumulator is a DIFFERENCE array, int32 diff[total_len + 1].  Everything a step leaves behind is a set of ranges -- a finished read's record is at most
// nine straight stretches, a searched read's pairs are runs --, and a range of found places [g_lo, g_hi] is +1 at g_lo and -1 at g_hi + 1, whichever way the
// offsets run in the read: two atomics per stretch, not one per k-mer.  depth[g] = diff[0] + ... + diff[g], made by a prefix sum when somebody asks
// (fin_depth_download).  The -1 lands inside the same unitig: its last k - 1 positions begin no k-mer; entry total_len is there for a place in the last of them
// that only a hand-made pair can name.  Arithmetic is modulo 2^32: exact while every position's true depth is below 2^32.
//
// What is read (the frame is fin_wave.h's).  Where the step left records, a lane per read:
//   kind 1 -- the record and ends_p[u] alone: the found stretches of fin_rec_walk.h.  Strand-slot order ascends in `off` whichever strand A is.  Two adds per
//             stretch.
//   kind 0 -- the wave scans the read's pairs, a row of 64 slots at a time.  fin_cover's run rule (greedy, not the segment rule: depth does not
//             care where a run is cut): a lane is a run head unless its (u, off) continues the lane before it by one step in the run's direction, ascending or
//             descending.  A ballot gives each head its run's length and the head issues the two adds.  A repeated identical pair is two runs and both count.  A
//             run that continues into the next row is cut at the boundary.
// Where the step left no records the flat pair array is scanned the same way, FIN_DEPTH_FLAT slots per wave.
//
// A slot outside the index -- a unitig number >= n_unitigs, or a place start(u) + off at or beyond total_len -- is decided PER SLOT, before runs are formed: it
// counts as absent and sets flag bit 1.  Half a range would poison every position behind it after the prefix sum; this way both ends of a run are known to be
// valid before either add is issued.  (As in fin_cover.hip the device check is weaker than fin_records_depth's: an offset that runs past its unitig's end but stays
// inside the text counts in the neighbouring unitig without a flag.  The search kernels never produce such a place.)
//
// Adds are 32-bit __hip_atomic_fetch_add, relaxed, agent scope, result unused.  Integer adds commute: the result is exact whatever order the lanes arrive in,
// and the same run added twice counts twice.  Nothing here writes anything but the difference array and the accumulator's flag word (bit 0: a step whose overflow
// list overran was offered -- nothing of it is added).  The add kernels read the step's overflow counter themselves: no host synchronisation.
//
// The download path: the prefix sum over a CHUNK of the difference array into a staging buffer of depths, in three passes -- tile sums, one block scanning the
// tile sums behind the carry of the chunks before (fin_blk_scan_kernel's pattern), apply -- and a statistics kernel over the staged depths.  No block waits for
// another.  The difference array is only read: the accumulator stays additive across downloads.  Element indices are uint64.
//
// Out of scope: partitioned indexes, fin_search_batch_multi, sums across ranks (the caller adds the downloaded arrays), the C++ mirror, saturation.  (Histograms, medians
// and other quantiles of the staged depths: fin_depthhist.hip.)
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_wave.h"

#define FIN_DEPTH_FLAT 4096u   // slots a wave scans in the flat form
#define FIN_DEPTH_STAT_P 8u    // positions a lane of the statistics kernel takes

namespace {
typedef unsigned long long ull;

__device__ __forceinline__ void depth_flag(uint32_t* flags, uint32_t bit) { (void)__hip_atomic_fetch_or(flags, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// positions [g_lo, g_end) each one deeper.  The caller has checked g_lo < g_end <= total_len
__device__ __forceinline__ void depth_range(int32_t* diff, uint64_t g_lo, uint64_t g_end) {
    (void)__hip_atomic_fetch_add(diff + g_lo, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(diff + g_end, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// slots [lo, hi) of the pair array, a row of 64 at a time, the whole wave.  Wave-converged.
__device__ __forceinline__ void depth_scan(const int2* pairs, uint64_t lo, uint64_t hi, const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len, int32_t* diff,
                                           uint32_t* flags) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = lo; base < hi; base += 64u) {
        const uint64_t j = base + lane;
        const bool act = j < hi;
        int2 p = make_int2(-1, -1);
        if (act) p = pairs[j];
        const uint32_t u = (uint32_t)p.x, off = (uint32_t)p.y;
        // the slot's own place, before any run is formed: a found slot that names no place of the index is flagged and counts as absent
        uint64_t g = 0;
        bool ok = false;
        if (act && u != 0xFFFFFFFFu) {
            if (u < n_unitigs) { g = (uint64_t)ends_p[u] + off; ok = g < total_len; }
            if (!ok) depth_flag(flags, 2u);
        }
        const uint32_t up = (uint32_t)__shfl_up((int)u, 1), offp = (uint32_t)__shfl_up((int)off, 1);
        const bool prev_ok = __shfl_up((int)ok, 1) != 0;
        const bool joins = ok && prev_ok && lane != 0u && u == up;
        const ull A = __ballot(act);
        const ull CU = __ballot(joins && off == offp + 1u), CD = __ballot(joins && off + 1u == offp);
        // a lane continues its predecessor's run only in that run's direction: one that steps up behind a lane that stepped down begins a run of its own
        const ull H = A & ~((CU & ~(CD << 1)) | (CD & ~(CU << 1)));   // run heads (absent slots are heads of nothing); bit 0 is set
        if (((H >> lane) & 1ull) && ok) {
            const ull above = lane == 63u ? 0ull : (H >> (lane + 1u)) << (lane + 1u);
            const uint32_t end = above ? (uint32_t)__ffsll((long long)above) - 1u : (uint32_t)__popcll(A);
            const uint32_t n = end - lane;                                 // 1 .. 64
            const bool down = n > 1u && ((CD >> (lane + 1u)) & 1ull);
            // every slot of the run is a valid place of unitig u, so the run's lowest place is at or above start(u) and its highest below total_len
            const uint64_t g_lo = down ? g - (n - 1u) : g;
            depth_range(diff, g_lo, g_lo + n);
        }
    }
}

// ---- the prefix sum's tiles: `tile` elements (1 .. 4096) per block of 256 threads, thread t holding elements [t * per, t * per + per) of the tile ----
// v[j] = element t * per + j of the tile that begins at `base` (0 beyond the tile or beyond n).  A whole tile of 4096 is loaded as four 16-byte words a thread
__device__ __forceinline__ void depth_tile_load(const uint32_t* x, uint64_t base, uint64_t n, uint32_t tile, uint32_t per, uint32_t v[16]) {
    if (tile == 4096u && base + 4096u <= n) {   // (base is a multiple of 4096 then, and x is 16-byte aligned)
        const uint4* q = (const uint4*)(x + base + (uint64_t)threadIdx.x * 16u);
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) { const uint4 w = q[j]; v[4 * j] = w.x; v[4 * j + 1] = w.y; v[4 * j + 2] = w.z; v[4 * j + 3] = w.w; }
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++) {
        const uint32_t i = threadIdx.x * per + j;
        v[j] = (j < per && i < tile && base + i < n) ? x[base + i] : 0u;
    }
}
}  // namespace

// A step that left records: a lane per read.  kind 1 -- the record's found stretches, two adds each; kind 0 -- the wave scans the read's pairs
__global__ __launch_bounds__(256) void fin_depth_rec_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_reads, uint32_t k,
                                                            const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len, int32_t* diff, uint32_t* flags,
                                                            const uint32_t* ovf_count, uint32_t ovf_cap) {
    if (fin_step_withheld(ovf_count, ovf_cap, flags)) return;
    const FinReadItem it = fin_read_item<false>(frec, out_offs, blockIdx.x * 256u + threadIdx.x, n_reads);
    if (it.kind == 1u && it.a.w != 0u) {
        const uint4 a = it.a;
        if (a.x >= n_unitigs) depth_flag(flags, 2u);
        else {
            const uint4 b = it.load_b();
            const uint32_t nk = a.w;
            const uint64_t g0 = (uint64_t)ends_p[a.x] + a.y;
            uint32_t lim = nk;   // strand slots [0, lim) name places of the text
            if (g0 + nk > total_len) { depth_flag(flags, 2u); lim = g0 < total_len ? (uint32_t)(total_len - g0) : 0u; }   // (the slots beyond it count as absent)
            // the found stretches (fin_rec_walk.h), each cut off at `lim`
            (void)sgm_rec_walk(a, b, k, [&](uint32_t, uint32_t from, uint32_t to) {
                if (to > lim) to = lim;
                if (from < to) depth_range(diff, g0 + from, g0 + to);
            });
        }
    }
    fin_each_searched_read(it, [&](int, uint64_t lo, uint64_t hi) { depth_scan(pairs, lo, hi, ends_p, n_unitigs, total_len, diff, flags); });
}

// A step that left no records: every slot of the pair array, FIN_DEPTH_FLAT consecutive slots per wave (runs then reach across reads, which depth does not mind)
__global__ __launch_bounds__(256) void fin_depth_flat_kernel(const int2* pairs, uint64_t n_pairs, const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len,
                                                             int32_t* diff, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap) {
    if (fin_step_withheld(ovf_count, ovf_cap, flags)) return;
    const uint64_t n_spans = (n_pairs + FIN_DEPTH_FLAT - 1u) / FIN_DEPTH_FLAT;
    for (uint64_t s = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); s < n_spans; s += (uint64_t)gridDim.x * 4u) {
        const uint64_t lo = s * FIN_DEPTH_FLAT, hi = lo + FIN_DEPTH_FLAT < n_pairs ? lo + FIN_DEPTH_FLAT : n_pairs;
        depth_scan(pairs, lo, hi, ends_p, n_unitigs, total_len, diff, flags);
    }
}

// ---- the prefix sum of one chunk: x[0 .. n) are the chunk's differences, tile_sum has a word per tile ----
// 1. tile_sum[b] = the sum of tile b
__global__ __launch_bounds__(256) void fin_depth_tile_sum_kernel(const uint32_t* x, uint64_t n, uint32_t tile, uint32_t per, uint32_t* tile_sum) {
    __shared__ uint32_t lds[4];
    uint32_t v[16];
    depth_tile_load(x, (uint64_t)blockIdx.x * tile, n, tile, per, v);
    uint32_t s = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++) s += v[j];
    uint32_t total = 0;
    (void)fin_block_exclusive4(s, lds, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}
// 2. one block: tile_sum[b] becomes what lies in front of tile b -- *carry (the chunks before this one) plus the tiles before it; *carry takes this chunk's sum in
__global__ __launch_bounds__(1024) void fin_depth_tile_scan_kernel(uint32_t* tile_sum, uint32_t n_tiles, uint32_t* carry) {
    __shared__ uint32_t lds[1024];
    const uint32_t per = (n_tiles + 1023u) / 1024u, b0 = threadIdx.x * per;
    const uint32_t c = *carry;
    uint32_t s = 0;
    for (uint32_t i = 0; i < per; i++) if (b0 + i < n_tiles) s += tile_sum[b0 + i];
    lds[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t y = threadIdx.x >= d ? lds[threadIdx.x - d] : 0u;
        __syncthreads();
        lds[threadIdx.x] += y;
        __syncthreads();
    }
    uint32_t at = c + lds[threadIdx.x] - s;
    for (uint32_t i = 0; i < per; i++) if (b0 + i < n_tiles) { const uint32_t t = tile_sum[b0 + i]; tile_sum[b0 + i] = at; at += t; }
    if (threadIdx.x == 1023u) *carry = c + lds[1023];   // (every thread read *carry before the first barrier)
}
// 3. depth[i] = tile_sum[b] + x[b * tile] + ... + x[i] for every element i of tile b
__global__ __launch_bounds__(256) void fin_depth_apply_kernel(const uint32_t* x, uint64_t n, uint32_t tile, uint32_t per, const uint32_t* tile_sum, uint32_t* depth) {
    __shared__ uint32_t lds[4];
    const uint64_t base = (uint64_t)blockIdx.x * tile;
    uint32_t v[16];
    depth_tile_load(x, base, n, tile, per, v);
    uint32_t s = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++) { s += v[j]; v[j] = s; }   // inclusive inside the thread
    const uint32_t before = tile_sum[blockIdx.x] + fin_block_exclusive4(s, lds, nullptr);
    if (tile == 4096u && base + 4096u <= n) {
        uint4* q = (uint4*)(depth + base + (uint64_t)threadIdx.x * 16u);
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) q[j] = make_uint4(before + v[4 * j], before + v[4 * j + 1], before + v[4 * j + 2], before + v[4 * j + 3]);
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++) {
        const uint32_t i = threadIdx.x * per + j;
        if (j < per && i < tile && base + i < n) depth[base + i] = before + v[j];
    }
}

// stats[u] += {sum, max, positions with depth >= min_depth} over depth[0 .. n), the depths of text positions g_base .. g_base + n: a lane takes FIN_DEPTH_STAT_P
// consecutive positions.  The first one's unitig is looked up in ends_p (the unitig u with ends_p[u] <= g < ends_p[u + 1], as fin_cover_count_kernel finds a
// word's); from there the lane walks, handing a unitig's share over when it crosses into the next.  A wave whose lanes all end in one unitig adds once.
__global__ __launch_bounds__(256) void fin_depth_stat_kernel(const uint32_t* depth, uint64_t g_base, uint64_t n, const uint32_t* ends_p, uint32_t n_unitigs,
                                                             uint32_t min_depth, FinDepthStat* stats) {
    const uint64_t i0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * FIN_DEPTH_STAT_P;
    const bool act = i0 < n;
    uint32_t u = 0, mx = 0, c = 0;
    ull s = 0;
    auto flush = [&](uint32_t uu, ull ss, uint32_t mm, uint32_t cc) {
        if (ss) (void)__hip_atomic_fetch_add(&stats[uu].sum, ss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (mm) (void)__hip_atomic_fetch_max(&stats[uu].max, mm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cc) (void)__hip_atomic_fetch_add(&stats[uu].n_at_least, cc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    if (act) {
        uint32_t d[FIN_DEPTH_STAT_P];
        const uint32_t m = n - i0 < FIN_DEPTH_STAT_P ? (uint32_t)(n - i0) : FIN_DEPTH_STAT_P;
        if (m == FIN_DEPTH_STAT_P) {   // (depth is 16-byte aligned and i0 a multiple of 8)
            const uint4 w0 = ((const uint4*)(depth + i0))[0], w1 = ((const uint4*)(depth + i0))[1];
            d[0] = w0.x; d[1] = w0.y; d[2] = w0.z; d[3] = w0.w; d[4] = w1.x; d[5] = w1.y; d[6] = w1.z; d[7] = w1.w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < FIN_DEPTH_STAT_P; j++) d[j] = j < m ? depth[i0 + j] : 0u;
        }
        const uint64_t g0 = g_base + i0;
        uint32_t lo = 0, hi = n_unitigs;   // the last u in [0, n_unitigs) with ends_p[u] <= g0 (ends_p[0] = 0)
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if ((uint64_t)ends_p[mid] <= g0) lo = mid; else hi = mid; }
        u = lo;
        uint64_t next = ends_p[u + 1];
#pragma unroll
        for (uint32_t j = 0; j < FIN_DEPTH_STAT_P; j++) {
            if (j < m) {
                while (g0 + j >= next && u + 1u < n_unitigs) { flush(u, s, mx, c); s = 0; mx = 0; c = 0; u++; next = ends_p[u + 1]; }
                s += d[j]; mx = d[j] > mx ? d[j] : mx; c += d[j] >= min_depth ? 1u : 0u;
            }
        }
    }
    // (lane 0 is idle only where the whole wave is: positions ascend with the lane)
    const uint32_t u0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)u);
    if (__ballot(act && u != u0) == 0ull) {
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) {
            s += __shfl_xor(s, dd);
            const uint32_t m2 = (uint32_t)__shfl_xor((int)mx, dd);
            mx = m2 > mx ? m2 : mx;
            c += (uint32_t)__shfl_xor((int)c, dd);
        }
        if ((threadIdx.x & 63u) == 0u && act) flush(u0, s, mx, c);
        return;
    }
    if (act) flush(u, s, mx, c);
}

// diff: int32[total_len + 1]; flags: one u32 (bit 0: a step without results was offered, bit 1: a unitig number or place outside the index).
// frec null: the flat form.  ovf_count (may be null) / ovf_cap: the step's overflow list, as batch_overrun_check reads it
extern "C" int fin_launch_depth_add(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint64_t n_pairs, uint32_t k, const uint32_t* ends_p,
                                    uint32_t n_unitigs, uint64_t total_len, void* diff, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap, hipStream_t stream) {
    if (n_reads == 0 || n_unitigs == 0 || total_len == 0) return 0;
    if (frec) {
        hipLaunchKernelGGL(fin_depth_rec_kernel, dim3((n_reads + 255u) / 256u), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs, n_reads, k,
                           ends_p, n_unitigs, total_len, (int32_t*)diff, flags, ovf_count, ovf_cap);
    } else {
        if (n_pairs == 0) return 0;
        const uint64_t want = ((n_pairs + FIN_DEPTH_FLAT - 1u) / FIN_DEPTH_FLAT + 3u) / 4u;
        hipLaunchKernelGGL(fin_depth_flat_kernel, dim3((uint32_t)(want < 65536u ? want : 65536u)), dim3(256), 0, stream, (const int2*)pairs, n_pairs, ends_p, n_unitigs,
                           total_len, (int32_t*)diff, flags, ovf_count, ovf_cap);
    }
    return (int)hipGetLastError();
}

extern "C" uint32_t fin_depth_max_tile(void) { return 4096u; }
extern "C" uint32_t fin_depth_max_chunk_tiles(void) { return 4096u; }

// depth[0 .. n) = *carry + the inclusive prefix sum of diff[0 .. n), one chunk: n <= tile * fin_depth_max_chunk_tiles(), 1 <= tile <= fin_depth_max_tile();
// tile_sum: a u32 per tile; *carry: the sum of everything in front of the chunk, moved on to the chunk's end.  diff and depth are 16-byte aligned.
extern "C" int fin_launch_depth_scan_chunk(const void* diff, uint64_t n, uint32_t tile, uint32_t* tile_sum, uint32_t* carry, uint32_t* depth, hipStream_t stream) {
    if (n == 0) return 0;
    if (tile == 0u || tile > 4096u || (n + tile - 1u) / tile > 4096u) return (int)hipErrorInvalidValue;
    const uint32_t n_tiles = (uint32_t)((n + tile - 1u) / tile), per = (tile + 255u) / 256u;
    hipLaunchKernelGGL(fin_depth_tile_sum_kernel, dim3(n_tiles), dim3(256), 0, stream, (const uint32_t*)diff, n, tile, per, tile_sum);
    hipLaunchKernelGGL(fin_depth_tile_scan_kernel, dim3(1), dim3(1024), 0, stream, tile_sum, n_tiles, carry);
    hipLaunchKernelGGL(fin_depth_apply_kernel, dim3(n_tiles), dim3(256), 0, stream, (const uint32_t*)diff, n, tile, per, (const uint32_t*)tile_sum, depth);
    return (int)hipGetLastError();
}

// stats: FinDepthStat[n_unitigs], zeroed by the caller before the first chunk; depth[0 .. n) are the depths of text positions g_base .. g_base + n (all below total_len)
extern "C" int fin_launch_depth_stats(const uint32_t* depth, uint64_t g_base, uint64_t n, const uint32_t* ends_p, uint32_t n_unitigs, uint32_t min_depth, void* stats,
                                      hipStream_t stream) {
    if (n == 0 || n_unitigs == 0) return 0;
    const uint64_t lanes = (n + FIN_DEPTH_STAT_P - 1u) / FIN_DEPTH_STAT_P;
    hipLaunchKernelGGL(fin_depth_stat_kernel, dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, stream, depth, g_base, n, ends_p, n_unitigs, min_depth,
                       (FinDepthStat*)stats);
    return (int)hipGetLastError();
}
