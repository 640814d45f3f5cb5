// fin_colors.hip -- COLOUR SETS per unitig and read PSEUDOALIGNMENT against them (include/finito_amd.h: fin_colors, fin_batch_add_colors, fin_read_pseudo,
// fin_batch_pseudoalign).  Where fin_classify.hip knows one label per unitig, this knows the SET of references a unitig occurs in, the common case
// in a graph built over many genomes.
//
// The matrix: uint64 bits[n_unitigs][W], W = ceil(n_colors / 64) <= 64; colour c of unitig u is bit c & 63 of bits[u * W + (c >> 6)]; bits at or above n_colors
// are 0.  Behind the matrix lies one flag word (bit 0: a step whose overflow list overran was offered to fin_batch_add_colors -- nothing of it is set).
//
// fin_col_add_kernel: every unitig in which the run found at least one k-mer gets bit `color`.  A lane per read (the frame is fin_wave.h's):
//   kind 1 -- the record lies in one unitig; if sgm_rec_walk gives a found slot, one plain load of the word and, if the bit is clear, one 64-bit atomic OR.
//   kind 0 -- the wave scans the read's pairs, a row of 64 slots at a time, the next row loaded ahead; a loop over the row's DISTINCT unitigs
//             (fin_each_distinct); the first lane of each does the load-then-OR.
// Between two resets bits are only ever set: whatever the plain load returns is a subset of the truth, a stale view costs a redundant OR, never a lost one.  OR is
// idempotent: adding a run twice changes nothing.  A unitig number at or above n_unitigs (the absent slot's 0xFFFFFFFF is one) is skipped.
//
// fin_col_pseudo_kernel: over a read's output slots, a found slot whose unitig has a non-empty row is COLOURED; cnt[c] = the coloured slots whose unitig has
// colour c; colour c is in the read's row iff cnt[c] >= 1 and 1000 * cnt[c] >= permille * n_coloured (64-bit).  permille 1000: the intersection over the coloured
// k-mers; 0: the union.  Invariant under reversing the slot order.  A lane per read:
//   kind 1 -- n found slots in unitig u: every cnt is n, so the row is bits[u] itself (n > 0), head {n, row non-empty ? n : 0, popcount, 0}.  The copies are
//             wave-cooperative: a ballot of the lanes whose row is a copy (or zero: kind 2, reads without pairs), then for each the wave moves the row, lane i
//             word i -- coalesced loads and stores.  W = 1: a lane moves its own read's word, which is coalesced as it is.
//   kind 0 -- the wave scans the read's pairs once, by rows, with the distinct-unitig loop, and keeps a table (unitig, count) in its registers, entry i in lane i
//             (FinUnitigTable).
//             At the read's end n_coloured = the counts of the entries with a non-empty row; then for each word w lane e gathers bits[u_e * W + w], a wave-uniform
//             loop over the entries broadcasts entry e's word and count, lane b adds the count if bit b is set: lane b holds cnt[64 w + b], and the output word is
//             ONE BALLOT of the threshold test, stored by one lane.
//   more than 64 distinct unitigs in one read -- the table is dropped; n_coloured comes from a rescan (a lane per slot looks at its unitig's row), then for each
//             word w the rows are scanned again: for each distinct unitig of a row its word w is broadcast and the lanes whose bit is set add the ballot's
//             popcount.  Counts are additive over rows: exact, at W + 1 rescans for a read that rare.
// No LDS, no atomics, no global scratch on the per-read result; every output word has one writer.  A slot whose unitig number is at or above n_unitigs counts as
// absent.
//
// fin_col_pseudo_sets_kernel: the same body over a COMPACT matrix (fin_colorsets.hip) -- every unitig number becomes set_of[u] as it is loaded
// (fin_wave.h: fin_row_key), bits = sets, n_unitigs = n_sets + 1, and the table is keyed by set id: counts are additive over the unitigs of one set, so only a
// read with more than 64 distinct SETS is rescanned.  Set 0 is the empty row: "coloured" needs no special case.
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_wave.h"

#define FIN_COL_BLK 256u   // reads per block: a lane per read

namespace {
typedef unsigned long long ull;

// bits[w] |= m: one plain load, the atomic only where the bit is clear.  The caller has checked that w is a word of the matrix
__device__ __forceinline__ void col_or(ull* bits, uint64_t w, ull m) {
    if ((__hip_atomic_load(bits + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m) == m) return;
    (void)__hip_atomic_fetch_or(bits + w, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// slots [lo, hi) of the pair array are one read's: bit `color` for every distinct unitig.  Wave-converged
__device__ __forceinline__ void col_add_scan(const int2* pairs, uint64_t lo, uint64_t hi, ull* bits, uint32_t W, uint32_t n_unitigs, uint32_t color) {
    const uint32_t lane = threadIdx.x & 63u;
    fin_each_pair_row(pairs, lo, hi, [&](uint64_t, uint64_t, int2 p) {
        const uint32_t u = (uint32_t)p.x;
        fin_each_distinct(u, u < n_unitigs, [&](int src, uint32_t uc, ull) {
            if ((int)lane == src) col_or(bits, (uint64_t)uc * W + (color >> 6), 1ull << (color & 63u));
        });
    });
}

// slots [lo, hi) are one read's: its row into out[0 .. W), its head {n_found, n_coloured, popcount of the row} returned in every lane.  Wave-converged.
// SETS: the rows are keyed by set id (fin_row_key): bits = sets, n_unitigs = n_sets + 1, set_of and n_u the map and the index's unitigs
template <bool SETS>
__device__ __forceinline__ uint4 col_pseudo_scan(const int2* pairs, uint64_t lo, uint64_t hi, const ull* bits, uint32_t W, uint32_t n_unitigs, uint32_t permille,
                                                 ull* out, const uint32_t* set_of, uint32_t n_u) {
    uint32_t n_found = 0;
    FinUnitigTable tab;
    fin_each_pair_row(pairs, lo, hi, [&](uint64_t, uint64_t, int2 p) {
        const uint32_t u = fin_row_key<SETS>((uint32_t)p.x, set_of, n_u);
        n_found += (uint32_t)__popcll(__ballot(u < n_unitigs));
        fin_each_distinct(u, u < n_unitigs, [&](int, uint32_t uc, ull m) { (void)tab.add(uc, (uint32_t)__popcll(m)); });
    });
    uint32_t n_colored = 0, pc = 0;
    if (!tab.over) {
        n_colored = fin_wave_sum(tab.colored(bits, W) ? tab.t_cnt : 0u);
        const uint64_t need = (uint64_t)permille * n_colored;
        for (uint32_t w = 0; w < W; w++) pc += fin_row_word(tab.word_counts(bits, W, w), need, true, out, w);
    } else {
        n_colored = fin_rescan_colored<SETS>(pairs, lo, hi, bits, W, n_unitigs, set_of, n_u);
        const uint64_t need = (uint64_t)permille * n_colored;
        for (uint32_t w = 0; w < W; w++) pc += fin_row_word(fin_rescan_word<SETS>(pairs, lo, hi, bits, W, n_unitigs, w, set_of, n_u), need, true, out, w);
    }
    return make_uint4(n_found, n_colored, pc, 0u);
}

// the body of fin_col_pseudo_kernel and, with SETS, of fin_col_pseudo_sets_kernel: there a kind-1 record's unitig becomes its set id as well
template <bool SETS>
__device__ __forceinline__ void col_pseudo_body(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_reads, uint32_t k, const ull* bits,
                                                uint32_t W, uint32_t n_unitigs, uint32_t permille, ull* rows, uint4* heads, const uint32_t* set_of, uint32_t n_u) {
    const uint32_t r = blockIdx.x * FIN_COL_BLK + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t r0 = r - lane;           // the wave's first read
    const FinReadItem it = fin_read_item<false>(frec, out_offs, r, n_reads);
    uint32_t u = 0, n = 0;                  // a kind-1 read's unitig and found slots
    if (it.kind == 1u && it.a.w != 0u && it.a.x < (SETS ? n_u : n_unitigs)) {
        (void)sgm_rec_walk(it.a, it.load_b(), k, [&](uint32_t, uint32_t from, uint32_t to) { n += to - from; });
        u = fin_row_key<SETS>(it.a.x, set_of, n_u);
    }
    const bool scanned = it.scanned();
    uint4 mine = make_uint4(0u, 0u, 0u, 0u);
    // ---- the rows that are a copy of one unitig's row, or zero ----
    if (W == 1u) {
        if (r < n_reads && !scanned) {
            const ull word = n != 0u ? bits[u] : 0ull;
            rows[r] = word;
            mine = make_uint4(n, word ? n : 0u, (uint32_t)__popcll(word), 0u);
        }
    } else {
        fin_each_lane(r < n_reads && !scanned, [&](int src) {
            const uint32_t us = fin_bcast(u, src), ns = fin_bcast(n, src);
            ull word = 0ull;
            if (lane < W) {
                if (ns != 0u) word = bits[(uint64_t)us * W + lane];
                rows[(uint64_t)(r0 + (uint32_t)src) * W + lane] = word;
            }
            const uint32_t pc = fin_wave_sum((uint32_t)__popcll(word));
            if ((int)lane == src) mine = make_uint4(n, pc ? n : 0u, pc, 0u);
        });
    }
    fin_each_searched_read(it, [&](int src, uint64_t lo, uint64_t hi) {
        const uint4 s = col_pseudo_scan<SETS>(pairs, lo, hi, bits, W, n_unitigs, permille, rows + (uint64_t)(r0 + (uint32_t)src) * W, set_of, n_u);
        if ((int)lane == src) mine = s;
    });
    if (r < n_reads) heads[r] = mine;
}

}  // namespace

// bits[u][color] = 1 for every unitig u in which the run found a k-mer.  frec null: the step left no records, every read is scanned.
__global__ __launch_bounds__(256) void fin_col_add_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_reads, uint32_t k, ull* bits,
                                                          uint32_t W, uint32_t n_unitigs, uint32_t color, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap) {
    if (fin_step_withheld(ovf_count, ovf_cap, flags)) return;
    const FinReadItem it = fin_read_item<false>(frec, out_offs, blockIdx.x * FIN_COL_BLK + threadIdx.x, n_reads);
    if (it.kind == 1u && it.a.w != 0u && it.a.x < n_unitigs) {
        uint32_t n = 0;
        (void)sgm_rec_walk(it.a, it.load_b(), k, [&](uint32_t, uint32_t from, uint32_t to) { n += to - from; });
        if (n != 0u) col_or(bits, (uint64_t)it.a.x * W + (color >> 6), 1ull << (color & 63u));
    }
    fin_each_searched_read(it, [&](int, uint64_t lo, uint64_t hi) { col_add_scan(pairs, lo, hi, bits, W, n_unitigs, color); });
}

// rows[r][0 .. W) = read r's colour row, heads[r] = {n_found, n_coloured, popcount, 0}.  frec null: the step left no records, every read is scanned.
__global__ __launch_bounds__(256) void fin_col_pseudo_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_reads, uint32_t k,
                                                             const ull* bits, uint32_t W, uint32_t n_unitigs, uint32_t permille, ull* rows, uint4* heads) {
    col_pseudo_body<false>(frec, out_offs, pairs, n_reads, k, bits, W, n_unitigs, permille, rows, heads, nullptr, 0u);
}
// the same over a compact matrix: sets uint64[(n_sets + 1) * W] and set_of[n_unitigs]; every unitig number becomes its set id as it is loaded
__global__ __launch_bounds__(256) void fin_col_pseudo_sets_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_reads, uint32_t k,
                                                                  const ull* sets, uint32_t W, uint32_t n_sets1, const uint32_t* set_of, uint32_t n_unitigs,
                                                                  uint32_t permille, ull* rows, uint4* heads) {
    col_pseudo_body<true>(frec, out_offs, pairs, n_reads, k, sets, W, n_sets1, permille, rows, heads, set_of, n_unitigs);
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
// the same over a compact matrix: sets uint64[(n_sets + 1) * W], row 0 empty; set_of: uint32[n_unitigs], each <= n_sets
extern "C" int fin_launch_pseudoalign_sets(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, const void* sets, uint32_t W,
                                           uint32_t n_sets, const uint32_t* set_of, uint32_t n_unitigs, uint32_t permille, void* rows, void* heads, hipStream_t stream) {
    const uint32_t nb = (n_reads + FIN_COL_BLK - 1u) / FIN_COL_BLK;
    if (nb == 0) return 0;
    hipLaunchKernelGGL(fin_col_pseudo_sets_kernel, dim3(nb), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs, n_reads, k, (const ull*)sets, W,
                       n_sets + 1u, set_of, n_unitigs, permille, (ull*)rows, (uint4*)heads);
    return (int)hipGetLastError();
}
