// fin_colors.hip -- COLOUR SETS per unitig and read PSEUDOALIGNMENT against them (include/finito_amd.h: fin_colors, fin_batch_add_colors, fin_read_pseudo,
// fin_batch_pseudoalign).  Where fin_classify.hip knows one label per unitig, this knows the SET of references a unitig occurs in, the common case
// in a graph built over many genomes.
//
// The matrix: uint64 bits[n_unitigs][W], W = ceil(n_colors / 64) <= 64; colour c of unitig u is bit c & 63 of bits[u * W + (c >> 6)]; bits at or above n_colors
// are 0.  Behind the matrix lies one flag word (bit 0: a step whose overflow list overran was offered to fin_batch_add_colors -- nothing of it is set).
//
// fin_col_add_kernel: every unitig in which the run found at least one k-mer gets bit `color`.  A lane per read:
//   kind 1 -- the record lies in one unitig; if sgm_rec_walk gives a found slot, one plain load of the word and, if the bit is clear, one 64-bit atomic OR.  The
//             read's pairs are never touched -- in text mode 2 they do not exist.
//   kind 2 -- nothing.
//   kind 0 -- (and every read where the step left no records) the wave scans the read's pairs through out_offs, a row of 64 slots at a time, the next row loaded
//             ahead; a loop over the row's DISTINCT unitigs (readlane of the first lane left, a ballot of the lanes with the same unitig); that first lane does
//             the load-then-OR.
// Between two resets bits are only ever set: whatever the plain load returns is a subset of the truth, a stale view costs a redundant OR, never a lost one.  OR is
// idempotent: adding a run twice changes nothing.  A unitig number at or above n_unitigs (the absent slot's 0xFFFFFFFF is one) is skipped.
//
// fin_col_pseudo_kernel: over a read's output slots, a found slot whose unitig has a non-empty row is COLOURED; cnt[c] = the coloured slots whose unitig has
// colour c; colour c is in the read's row iff cnt[c] >= 1 and 1000 * cnt[c] >= permille * n_coloured (64-bit).  permille 1000: the intersection over the coloured
// k-mers; 0: the union.  Invariant under reversing the slot order.  A lane per read:
//   kind 1 -- n found slots in unitig u: every cnt is n, so the row is bits[u] itself (n > 0), head {n, row non-empty ? n : 0, popcount, 0}.  The copies are
//             wave-cooperative: a ballot of the lanes whose row is a copy (or zero: kind 2, reads without pairs), then for each the wave moves the row, lane i
//             word i -- coalesced loads and stores.  W = 1: a lane moves its own read's word, which is coalesced as it is.
//   kind 0 -- the wave scans the read's pairs once, by rows, with the distinct-unitig loop, and keeps a table (unitig, count) in its registers, entry i in lane i.
//             At the read's end n_coloured = the counts of the entries with a non-empty row; then for each word w lane e gathers bits[u_e * W + w], a wave-uniform
//             loop over the entries broadcasts entry e's word and count, lane b adds the count if bit b is set: lane b holds cnt[64 w + b], and the output word is
//             ONE BALLOT of the threshold test, stored by one lane.
//   more than 64 distinct unitigs in one read -- the table is dropped; n_coloured comes from a rescan (a lane per slot looks at its unitig's row), then for each
//             word w the rows are scanned again: for each distinct unitig of a row its word w is broadcast and the lanes whose bit is set add the ballot's
//             popcount.  Counts are additive over rows: exact, at W + 1 rescans for a read that rare.
// No LDS, no atomics, no global scratch on the per-read result; every output word has one writer.  A slot whose unitig number is at or above n_unitigs counts as
// absent.
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_rec_walk.h"

#define FIN_COL_BLK 256u   // reads per block: a lane per read

namespace {
typedef unsigned long long ull;

__device__ __forceinline__ uint32_t col_bcast(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, src); }
__device__ __forceinline__ uint64_t col_bcast64(uint64_t v, int src) { return ((uint64_t)col_bcast((uint32_t)(v >> 32), src) << 32) | col_bcast((uint32_t)v, src); }
__device__ __forceinline__ uint32_t col_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

// bits[w] |= m: one plain load, the atomic only where the bit is clear.  The caller has checked that w is a word of the matrix
__device__ __forceinline__ void col_or(ull* bits, uint64_t w, ull m) {
    if ((__hip_atomic_load(bits + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m) == m) return;
    (void)__hip_atomic_fetch_or(bits + w, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// slots [lo, hi) of the pair array are one read's: bit `color` for every distinct unitig.  Wave-converged
__device__ __forceinline__ void col_add_scan(const int2* pairs, uint64_t lo, uint64_t hi, ull* bits, uint32_t W, uint32_t n_unitigs, uint32_t color) {
    const uint32_t lane = threadIdx.x & 63u;
    int2 pn = make_int2(-1, -1);            // the row to come, loaded a row ahead
    if (lo + lane < hi) pn = pairs[lo + lane];
    for (uint64_t base = lo; base < hi; base += 64u) {
        const uint64_t j = base + lane;
        const int2 p = pn;                  // (-1,-1) in a lane beyond the read's end
        pn = make_int2(-1, -1);
        if (j + 64u < hi) pn = pairs[j + 64u];
        const uint32_t u = (uint32_t)p.x;
        ull rem = __ballot(u < n_unitigs);
        while (rem) {
            const int src = __ffsll((long long)rem) - 1;
            const uint32_t uc = col_bcast(u, src);
            rem &= ~__ballot(u == uc);
            if ((int)lane == src) col_or(bits, (uint64_t)uc * W + (color >> 6), 1ull << (color & 63u));
        }
    }
}

// slots [lo, hi) are one read's: its row into out[0 .. W), its head {n_found, n_coloured, popcount of the row} returned in every lane.  Wave-converged
__device__ __forceinline__ uint4 col_pseudo_scan(const int2* pairs, uint64_t lo, uint64_t hi, const ull* bits, uint32_t W, uint32_t n_unitigs, uint32_t permille,
                                                 ull* out) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t n_found = 0, n_ent = 0;        // the table: entry i < n_ent in lane i
    uint32_t t_u = 0, t_cnt = 0;
    bool over = false;                      // more than 64 distinct unitigs: the table is dropped
    {
        int2 pn = make_int2(-1, -1);
        if (lo + lane < hi) pn = pairs[lo + lane];
        for (uint64_t base = lo; base < hi; base += 64u) {
            const uint64_t j = base + lane;
            const int2 p = pn;
            pn = make_int2(-1, -1);
            if (j + 64u < hi) pn = pairs[j + 64u];
            const uint32_t u = (uint32_t)p.x;
            ull rem = __ballot(u < n_unitigs);
            n_found += (uint32_t)__popcll(rem);
            while (rem && !over) {          // the row's distinct unitigs, one item each
                const int src = __ffsll((long long)rem) - 1;
                const uint32_t uc = col_bcast(u, src);
                const ull m = __ballot(u == uc);
                rem &= ~m;
                const bool mine = lane < n_ent && t_u == uc;
                if (__ballot(mine)) { if (mine) t_cnt += (uint32_t)__popcll(m); }
                else if (n_ent < 64u) {
                    if (lane == n_ent) { t_u = uc; t_cnt = (uint32_t)__popcll(m); }
                    n_ent++;
                } else over = true;
            }
        }
    }
    uint32_t n_colored = 0, pc = 0;
    if (!over) {
        const bool live = lane < n_ent;
        const ull* row = bits + (uint64_t)t_u * W;   // (t_u = 0 in a lane without an entry: never read)
        bool ne = false;
        for (uint32_t w = 0; w < W; w++) if (live && row[w] != 0ull) ne = true;
        n_colored = col_wave_sum(live && ne ? t_cnt : 0u);
        const uint64_t need = (uint64_t)permille * n_colored;
        for (uint32_t w = 0; w < W; w++) {
            const ull word = live ? row[w] : 0ull;
            uint32_t cnt = 0;
            for (uint32_t e = 0; e < n_ent; e++) {   // wave-uniform
                const ull we = col_bcast64(word, (int)e);
                const uint32_t ce = col_bcast(t_cnt, (int)e);
                if ((we >> lane) & 1ull) cnt += ce;
            }
            const ull o = __ballot(cnt >= 1u && 1000ull * cnt >= need);
            if (lane == 0u) out[w] = o;
            pc += (uint32_t)__popcll(o);
        }
    } else {
        // n_coloured: a lane per slot looks at its unitig's row
        for (uint64_t base = lo; base < hi; base += 64u) {
            const uint64_t j = base + lane;
            uint32_t u = 0xFFFFFFFFu;
            if (j < hi) u = (uint32_t)pairs[j].x;
            bool ne = false;
            if (u < n_unitigs) for (uint32_t w = 0; w < W; w++) if (bits[(uint64_t)u * W + w] != 0ull) ne = true;
            n_colored += (uint32_t)__popcll(__ballot(ne));
        }
        const uint64_t need = (uint64_t)permille * n_colored;
        for (uint32_t w = 0; w < W; w++) {
            uint32_t cnt = 0;
            for (uint64_t base = lo; base < hi; base += 64u) {
                const uint64_t j = base + lane;
                uint32_t u = 0xFFFFFFFFu;
                if (j < hi) u = (uint32_t)pairs[j].x;
                ull word = 0ull;
                if (u < n_unitigs) word = bits[(uint64_t)u * W + w];
                ull rem = __ballot(u < n_unitigs);
                while (rem) {
                    const int src = __ffsll((long long)rem) - 1;
                    const uint32_t uc = col_bcast(u, src);
                    const ull m = __ballot(u == uc);
                    rem &= ~m;
                    const ull we = col_bcast64(word, src);
                    if ((we >> lane) & 1ull) cnt += (uint32_t)__popcll(m);
                }
            }
            const ull o = __ballot(cnt >= 1u && 1000ull * cnt >= need);
            if (lane == 0u) out[w] = o;
            pc += (uint32_t)__popcll(o);
        }
    }
    return make_uint4(n_found, n_colored, pc, 0u);
}

}  // namespace

// bits[u][color] = 1 for every unitig u in which the run found a k-mer.  frec null: the step left no records, every read is scanned.
__global__ __launch_bounds__(256) void fin_col_add_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_reads, uint32_t k, ull* bits,
                                                          uint32_t W, uint32_t n_unitigs, uint32_t color, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap) {
    if (fin_step_withheld(ovf_count, ovf_cap, flags)) return;
    const uint32_t r = blockIdx.x * FIN_COL_BLK + threadIdx.x;
    uint32_t kind = 2u;
    uint64_t p_lo = 0, p_hi = 0;
    if (r < n_reads) {
        kind = 0u;
        if (frec) {
            const uint4 a = ((const uint4*)(frec + r))[0];   // u, off0, meta, nk
            kind = a.z >> 16;
            if (kind == 1u && a.w != 0u && a.x < n_unitigs) {
                const uint4 b = ((const uint4*)(frec + r))[1];
                uint32_t n = 0;
                (void)sgm_rec_walk(a, b, k, [&](uint32_t, uint32_t from, uint32_t to) { n += to - from; });
                if (n != 0u) col_or(bits, (uint64_t)a.x * W + (color >> 6), 1ull << (color & 63u));
            }
        }
        if (kind == 0u) { p_lo = out_offs[r]; p_hi = out_offs[r + 1]; }
    }
    // ---- the searched reads' pairs: the wave takes its lanes' reads one after the other ----
    ull todo = __ballot(kind == 0u && p_hi > p_lo);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        col_add_scan(pairs, col_bcast64(p_lo, src), col_bcast64(p_hi, src), bits, W, n_unitigs, color);
    }
}

// rows[r][0 .. W) = read r's colour row, heads[r] = {n_found, n_coloured, popcount, 0}.  frec null: the step left no records, every read is scanned.
__global__ __launch_bounds__(256) void fin_col_pseudo_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_reads, uint32_t k,
                                                             const ull* bits, uint32_t W, uint32_t n_unitigs, uint32_t permille, ull* rows, uint4* heads) {
    const uint32_t r = blockIdx.x * FIN_COL_BLK + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t r0 = r - lane;           // the wave's first read
    uint32_t kind = 2u;
    uint64_t p_lo = 0, p_hi = 0;
    uint32_t u = 0, n = 0;                  // a kind-1 read's unitig and found slots
    if (r < n_reads) {
        kind = 0u;
        if (frec) {
            const uint4 a = ((const uint4*)(frec + r))[0];   // u, off0, meta, nk
            kind = a.z >> 16;
            if (kind == 1u && a.w != 0u && a.x < n_unitigs) {
                const uint4 b = ((const uint4*)(frec + r))[1];
                (void)sgm_rec_walk(a, b, k, [&](uint32_t, uint32_t from, uint32_t to) { n += to - from; });
                u = a.x;
            }
        }
        if (kind == 0u) { p_lo = out_offs[r]; p_hi = out_offs[r + 1]; }
    }
    const bool scanned = kind == 0u && p_hi > p_lo;
    uint4 mine = make_uint4(0u, 0u, 0u, 0u);
    // ---- the rows that are a copy of one unitig's row, or zero ----
    if (W == 1u) {
        if (r < n_reads && !scanned) {
            const ull word = n != 0u ? bits[u] : 0ull;
            rows[r] = word;
            mine = make_uint4(n, word ? n : 0u, (uint32_t)__popcll(word), 0u);
        }
    } else {
        ull copy = __ballot(r < n_reads && !scanned);
        while (copy) {
            const int src = __ffsll((long long)copy) - 1;
            copy &= copy - 1ull;
            const uint32_t us = col_bcast(u, src), ns = col_bcast(n, src);
            ull word = 0ull;
            if (lane < W) {
                if (ns != 0u) word = bits[(uint64_t)us * W + lane];
                rows[(uint64_t)(r0 + (uint32_t)src) * W + lane] = word;
            }
            const uint32_t pc = col_wave_sum((uint32_t)__popcll(word));
            if ((int)lane == src) mine = make_uint4(n, pc ? n : 0u, pc, 0u);
        }
    }
    // ---- the searched reads' pairs: the wave takes its lanes' reads one after the other ----
    ull todo = __ballot(scanned);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const uint4 s = col_pseudo_scan(pairs, col_bcast64(p_lo, src), col_bcast64(p_hi, src), bits, W, n_unitigs, permille, rows + (uint64_t)(r0 + (uint32_t)src) * W);
        if ((int)lane == src) mine = s;
    }
    if (r < n_reads) heads[r] = mine;
}

// bits: uint64[n_unitigs * W]; flags: one u32 (bit 0: a step without results was offered).  frec null: every read is scanned.  ovf_count (may be null) / ovf_cap:
// the step's overflow list, as batch_overrun_check reads it.  color < 64 W is the caller's to check
extern "C" int fin_launch_colors_add(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, void* bits, uint32_t W,
                                     uint32_t n_unitigs, uint32_t color, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap, hipStream_t stream) {
    const uint32_t nb = (n_reads + FIN_COL_BLK - 1u) / FIN_COL_BLK;
    if (nb == 0 || n_unitigs == 0 || color >= 64u * W) return 0;
    hipLaunchKernelGGL(fin_col_add_kernel, dim3(nb), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs, n_reads, k, (ull*)bits, W, n_unitigs,
                       color, flags, ovf_count, ovf_cap);
    return (int)hipGetLastError();
}
// rows: uint64[n_reads * W]; heads: 16 bytes per read
extern "C" int fin_launch_pseudoalign(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, const void* bits, uint32_t W,
                                      uint32_t n_unitigs, uint32_t permille, void* rows, void* heads, hipStream_t stream) {
    const uint32_t nb = (n_reads + FIN_COL_BLK - 1u) / FIN_COL_BLK;
    if (nb == 0) return 0;
    hipLaunchKernelGGL(fin_col_pseudo_kernel, dim3(nb), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs, n_reads, k, (const ull*)bits, W,
                       n_unitigs, permille, (ull*)rows, (uint4*)heads);
    return (int)hipGetLastError();
}
