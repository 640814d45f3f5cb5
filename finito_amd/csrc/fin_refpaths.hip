// fin_refpaths.hip -- REFERENCE COORDINATES: per-position products of the unitig text lifted onto the sequences whose paths through the unitig set are known
// (include/finito_amd.h: REFERENCE COORDINATES, fin_refpaths_depth, fin_refpaths_lift_variants).  A path set is the canonical segments of 4.10 of
// n_seqs sequences, seg_offs[n_seqs + 1] delimiting them; segment {u, off, slot, len}, n = |len|, puts the sequence's slot slot + j at text position
// g = start(u) + off + j (len > 0) or start(u) + off - j (len < 0), 0 <= j < n.
//
// NO SCRATCH; NO LANE WAITS FOR ANOTHER LANE'S STORE; every loop bound is a kernel argument or wave-uniform; integer atomics only, so every sum is exact in any order.
//   fin_rp_tiles_kernel      cnt[i] = the tiles of segment i, ceil(n / tile), at least 1 (a segment of no slot is invalid: its one tile says so), and the sums per
//                            block of 256 segments; fin_launch_blk_scan makes the blocks' offsets; fin_rp_tile_offs_kernel the exclusive prefix tile_offs[n_segs + 1].
//   fin_rp_depth_kernel      a WAVE PER TILE.  The wave finds its segment by binary search in tile_offs (wave-uniform loads, as the spectrum kernel finds a unitig
//                            in ends_p) and the segment's sequence by binary search in seg_offs.  THE GUARD comes before any load of the depth: u < n_unitigs, n >= 1,
//                            and the offsets inside nk(u) by the validity rule -- an invalid segment adds nothing and sets the flag word; no address outside
//                            depth[0 .. total_len) is formed.  Then the tile goes by 64 slots a step: lane l loads depth[g] at consecutive addresses, ascending for a
//                            forward segment, descending for a reverse one -- one coalesced 256-byte request either way.  A step that lies in ONE window (decided from
//                            its first and last slot: wave-uniform) sums its three numbers in a butterfly and lane 0 issues one 64-bit add and two 32-bit adds.  A
//                            step that straddles a window boundary lets EVERY LANE ADD FOR ITSELF (zero sums and zero counts are not issued): at window = 1 that is
//                            every step, up to three atomics per slot into 16 bytes nobody else touches; at window = 1000 one step in sixteen.  Run heads were not
//                            built.
//   fin_rp_var_g_kernel      g[i] = ends_p[u_i] + off_i of the uploaded variants (the host has checked them: ascending, inside the index).
//   fin_rp_var_kernel<WRITE> a LANE PER SEGMENT, the same guard.  The segment's BASE interval of the text is [start(u) + off, start(u) + off + n + k - 2] forward,
//                            [start(u) + off - n + 1, start(u) + off + k - 1] reverse; two binary searches in g[] give the variants inside.  WRITE false: cnt[i] and
//                            the block sums; WRITE true: the block's exclusive prefix behind blk_off, then the records {seq, pos, var, flags}, ascending in g for a
//                            forward segment and descending for a reverse one, so that pos ascends.  A segment with very many candidates is written serially by its
//                            lane: not tuned here.
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_nk.h"
#include "fin_wave.h"

#define FIN_RP_BLK 256u

namespace {
typedef unsigned long long ull;

__device__ __forceinline__ void rp_flag(uint32_t* flags) { (void)__hip_atomic_fetch_or(flags, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the validity rule's clauses that the index decides: 0 <= u < n_unitigs, n >= 1, every offset of the segment a k-mer start of u
__device__ __forceinline__ bool rp_valid(uint4 s, const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len, uint32_t k, uint32_t& n) {
    const int len = (int)s.w;
    n = len < 0 ? 0u - (uint32_t)len : (uint32_t)len;
    if (s.x >= n_unitigs || n == 0u || (int)s.y < 0) return false;
    const uint32_t nk = fin_unitig_nk(ends_p, s.x, n_unitigs, total_len, k);
    if (len > 0) return (uint64_t)s.y + n <= nk;
    return s.y >= n - 1u && s.y < nk;
}

// the last i in [0, n) with a[i] <= x (a[0] <= x is the caller's); wave-uniform where x is
__device__ __forceinline__ uint64_t rp_last_le(const uint64_t* a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1u) { const uint64_t mid = lo + (hi - lo) / 2u; if (a[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}
// the first i in [0, n] with g[i] >= x
__device__ __forceinline__ uint64_t rp_first_ge(const uint64_t* g, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2u; if (g[mid] < x) lo = mid + 1u; else hi = mid; }
    return lo;
}
}  // namespace

__global__ __launch_bounds__(256) void fin_rp_tiles_kernel(const uint4* segs, uint64_t n_segs, uint32_t tile, uint32_t* cnt, uint32_t* blk_sum) {
    __shared__ uint32_t lds_w[4];
    const uint64_t i = (uint64_t)blockIdx.x * FIN_RP_BLK + threadIdx.x;
    uint32_t mine = 0;
    if (i < n_segs) {
        const int len = (int)segs[i].w;
        const uint32_t n = len < 0 ? 0u - (uint32_t)len : (uint32_t)len;
        mine = n == 0u ? 1u : (uint32_t)(((uint64_t)n + tile - 1u) / tile);
        cnt[i] = mine;
    }
    const uint32_t s = fin_block_sum4(mine, lds_w);
    if (threadIdx.x == 0) blk_sum[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void fin_rp_tile_offs_kernel(const uint32_t* cnt, uint64_t n_segs, const uint64_t* blk_off, uint64_t* tile_offs) {
    __shared__ uint32_t lds_w[4];
    const uint64_t i = (uint64_t)blockIdx.x * FIN_RP_BLK + threadIdx.x;
    const uint32_t mine = i < n_segs ? cnt[i] : 0u;
    const uint64_t at = blk_off[blockIdx.x] + fin_block_exclusive4(mine, lds_w, nullptr);
    if (i < n_segs) tile_offs[i] = at;
    if (i == n_segs - 1u) tile_offs[n_segs] = at + mine;
}

// a wave per tile; win: {uint64 depth_sum; uint32 in_graph; uint32 covered} per window, zeroed by the caller; floor = max(min_depth, 1)
__global__ __launch_bounds__(256) void fin_rp_depth_kernel(const uint4* segs, uint64_t n_segs, const uint64_t* seg_offs, uint64_t n_seqs, const uint64_t* tile_offs,
                                                           uint64_t n_tiles, uint32_t tile, const uint64_t* win_offs, uint32_t window, uint32_t floor,
                                                           const uint32_t* depth, const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len, uint32_t k, ull* win,
                                                           uint32_t* flags) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t t = (uint64_t)blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (t >= n_tiles) return;   // wave-uniform
    const uint64_t si = rp_last_le(tile_offs, n_segs, t);
    const uint4 s = segs[si];
    uint32_t n;
    if (!rp_valid(s, ends_p, n_unitigs, total_len, k, n)) { if (lane == 0u) rp_flag(flags); return; }
    const uint64_t seq = rp_last_le(seg_offs, n_seqs, si);   // the last sequence whose segments begin at or before si (a sequence without segments shares its offset with the next)
    const bool fwd = (int)s.w > 0;
    const uint64_t g0 = (uint64_t)ends_p[s.x] + s.y, w0 = win_offs[seq];
    // ... and the clause the sequence decides, as far as an address depends on it: the segment's last slot lies in one of its sequence's windows.  (No public
    // route leads here: fin_batch_segments cuts segments out of a read's own slots and fin_refpaths_upload checks slot + n <= seq_nk on the host.)
    if ((uint64_t)s.z + n > 0xFFFFFFFFull || w0 + (s.z + n - 1u) / window >= win_offs[seq + 1u]) { if (lane == 0u) rp_flag(flags); return; }
    const uint32_t i0 = (uint32_t)(t - tile_offs[si]) * tile, i1 = n - i0 < tile ? n : i0 + tile;   // the tile's slots [i0, i1) of the segment
    for (uint32_t base = i0; base < i1; base += 64u) {   // wave-uniform
        const uint32_t i = base + lane;
        const bool act = i < i1;
        uint32_t d = 0;
        if (act) d = depth[fwd ? g0 + i : g0 - i];
        const uint32_t last = (i1 - base < 64u ? i1 - base : 64u) - 1u;
        const uint32_t wa = (s.z + base) / window, wb = (s.z + base + last) / window;
        const uint32_t cov = act && d >= floor ? 1u : 0u;
        if (wa == wb) {
            const ull sum = fin_wave_sum64((ull)d);
            const uint32_t c = fin_wave_sum(cov);
            if (lane == 0u) {
                ull* const o = win + (w0 + wa) * 2u;
                if (sum) (void)__hip_atomic_fetch_add(o, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                (void)__hip_atomic_fetch_add((uint32_t*)(o + 1), last + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (c) (void)__hip_atomic_fetch_add((uint32_t*)(o + 1) + 1, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else if (act) {
            ull* const o = win + (w0 + (s.z + i) / window) * 2u;
            if (d) (void)__hip_atomic_fetch_add(o, (ull)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add((uint32_t*)(o + 1), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cov) (void)__hip_atomic_fetch_add((uint32_t*)(o + 1) + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// vars: {u, off, cover, ref, alt[4]} of 32 bytes each
__global__ __launch_bounds__(256) void fin_rp_var_g_kernel(const uint4* vars, uint64_t n, const uint32_t* ends_p, uint64_t* g) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) { const uint4 v = vars[2u * i]; g[i] = (uint64_t)ends_p[v.x] + v.y; }
}

template <bool WRITE>
__global__ __launch_bounds__(256) void fin_rp_var_kernel(const uint4* segs, uint64_t n_segs, const uint64_t* seg_offs, uint64_t n_seqs, const uint64_t* g, uint64_t n_vars,
                                                         const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len, uint32_t k, uint32_t* cnt, uint32_t* blk_sum,
                                                         const uint64_t* blk_off, uint4* out, uint32_t* flags) {
    __shared__ uint32_t lds_w[4];
    const uint64_t si = (uint64_t)blockIdx.x * FIN_RP_BLK + threadIdx.x;
    uint32_t mine = 0, n = 0;
    uint64_t j0 = 0, x0 = 0;
    uint4 s = make_uint4(0u, 0u, 0u, 0u);
    bool ok = false;
    if (si < n_segs) {
        s = segs[si];
        ok = rp_valid(s, ends_p, n_unitigs, total_len, k, n);
        if (!ok) rp_flag(flags);
        else {
            // the base interval [x0, x1] of the text: inside unitig u, since every offset of the segment is a k-mer start of it
            const uint64_t st = (uint64_t)ends_p[s.x] + s.y;
            x0 = (int)s.w > 0 ? st : st - (n - 1u);
            const uint64_t x1 = x0 + n + k - 2u;
            j0 = rp_first_ge(g, n_vars, x0);
            const uint64_t j1 = rp_first_ge(g, n_vars, x1 + 1u);
            mine = (uint32_t)(j1 - j0);   // (fewer than n + k - 1 <= 2^32: the variants ascend strictly)
        }
    }
    if (!WRITE) {
        if (si < n_segs) cnt[si] = mine;
        const uint32_t sum = fin_block_sum4(mine, lds_w);
        if (threadIdx.x == 0) blk_sum[blockIdx.x] = sum;
        return;
    }
    const uint64_t at = blk_off[blockIdx.x] + fin_block_exclusive4(mine, lds_w, nullptr);
    if (mine == 0u) return;
    const uint32_t seq = (uint32_t)rp_last_le(seg_offs, n_seqs, si);
    const bool fwd = (int)s.w > 0;
    for (uint32_t q = 0; q < mine; q++) {   // a lane's own count: the lanes of a wave leave the loop one by one, nobody waits for anybody
        const uint64_t j = fwd ? j0 + q : j0 + (mine - 1u - q);
        const uint32_t x = (uint32_t)(g[j] - x0);   // 0 .. n + k - 2 along the text
        const uint32_t pos = s.z + (fwd ? x : n + k - 2u - x);
        out[at + q] = make_uint4(seq, pos, (uint32_t)j, fwd ? 0u : 1u);
    }
}

// slots per tile: option "refpaths_tile" rounded up to a multiple of 64, or (0) 4096 (a segment has at most 2^31 slots: at most 2^19 tiles of it)
extern "C" uint32_t fin_rp_tile(uint32_t refpaths_tile) {
    const uint64_t t = refpaths_tile ? refpaths_tile : 4096u;
    return (uint32_t)((t + 63u) / 64u * 64u);
}
extern "C" uint32_t fin_rp_blocks(uint64_t n_segs) { return (uint32_t)((n_segs + FIN_RP_BLK - 1u) / FIN_RP_BLK); }

extern "C" int fin_launch_rp_tiles(const void* segs, uint64_t n_segs, uint32_t tile, uint32_t* cnt, uint32_t* blk_sum, uint64_t* blk_off, uint64_t* tile_offs,
                                   uint64_t* total, hipStream_t stream) {
    if (n_segs == 0 || n_segs >= (1ull << 39) || tile == 0u) return (int)hipErrorInvalidValue;
    const uint32_t nb = fin_rp_blocks(n_segs);
    hipLaunchKernelGGL(fin_rp_tiles_kernel, dim3(nb), dim3(256), 0, stream, (const uint4*)segs, n_segs, tile, cnt, blk_sum);
    const int rc = fin_launch_blk_scan(blk_sum, nb, blk_off, total, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(fin_rp_tile_offs_kernel, dim3(nb), dim3(256), 0, stream, (const uint32_t*)cnt, n_segs, (const uint64_t*)blk_off, tile_offs);
    return (int)hipGetLastError();
}

extern "C" int fin_launch_rp_depth(const void* segs, uint64_t n_segs, const uint64_t* seg_offs, uint64_t n_seqs, const uint64_t* tile_offs, uint64_t n_tiles,
                                   uint32_t tile, const uint64_t* win_offs, uint32_t window, uint32_t min_depth, const uint32_t* depth, const uint32_t* ends_p,
                                   uint32_t n_unitigs, uint64_t total_len, uint32_t k, void* win, uint32_t* flags, hipStream_t stream) {
    if (n_tiles == 0) return 0;
    if (n_segs == 0 || n_seqs == 0 || window == 0u || tile == 0u || (tile & 63u) || n_tiles >= (1ull << 33)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fin_rp_depth_kernel, dim3((uint32_t)((n_tiles + 3u) / 4u)), dim3(256), 0, stream, (const uint4*)segs, n_segs, seg_offs, n_seqs, tile_offs, n_tiles,
                       tile, win_offs, window, min_depth ? min_depth : 1u, depth, ends_p, n_unitigs, total_len, k, (ull*)win, flags);
    return (int)hipGetLastError();
}

extern "C" int fin_launch_rp_var_g(const void* vars, uint64_t n, const uint32_t* ends_p, uint64_t* g, hipStream_t stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(fin_rp_var_g_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, (const uint4*)vars, n, ends_p, g);
    return (int)hipGetLastError();
}

extern "C" int fin_launch_rp_var_count(const void* segs, uint64_t n_segs, const uint64_t* g, uint64_t n_vars, const uint32_t* ends_p, uint32_t n_unitigs,
                                       uint64_t total_len, uint32_t k, uint32_t* cnt, uint32_t* blk_sum, uint64_t* blk_off, uint64_t* total, uint32_t* flags,
                                       hipStream_t stream) {
    if (n_segs == 0 || n_segs >= (1ull << 39)) return (int)hipErrorInvalidValue;
    const uint32_t nb = fin_rp_blocks(n_segs);
    hipLaunchKernelGGL(fin_rp_var_kernel<false>, dim3(nb), dim3(256), 0, stream, (const uint4*)segs, n_segs, (const uint64_t*)nullptr, (uint64_t)0, g, n_vars, ends_p,
                       n_unitigs, total_len, k, cnt, blk_sum, (const uint64_t*)nullptr, (uint4*)nullptr, flags);
    return fin_launch_blk_scan(blk_sum, nb, blk_off, total, stream);
}

extern "C" int fin_launch_rp_var_write(const void* segs, uint64_t n_segs, const uint64_t* seg_offs, uint64_t n_seqs, const uint64_t* g, uint64_t n_vars,
                                       const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len, uint32_t k, const uint64_t* blk_off, void* out, uint32_t* flags,
                                       hipStream_t stream) {
    if (n_segs == 0 || n_seqs == 0 || n_segs >= (1ull << 39)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fin_rp_var_kernel<true>, dim3(fin_rp_blocks(n_segs)), dim3(256), 0, stream, (const uint4*)segs, n_segs, seg_offs, n_seqs, g, n_vars, ends_p,
                       n_unitigs, total_len, k, (uint32_t*)nullptr, (uint32_t*)nullptr, blk_off, (uint4*)out, flags);
    return (int)hipGetLastError();
}
