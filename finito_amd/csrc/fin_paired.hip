// fin_paired.hip -- PAIRED-END pseudoalignment: one colour row per FRAGMENT (include/finito_amd.h: fin_pair_pseudo, fin_batch_pseudoalign_paired).
// A batch of 2F reads holds F fragments, fragment f = reads 2f (first mate) and 2f + 1 (second mate).  The fragment's slots are the output slots of both mates
// together, and fin_colors.hip's definition is applied to that pooled list word for word: a found slot whose unitig has a non-empty row is COLOURED; cnt[c] = the
// coloured slots of either mate whose unitig has colour c; colour c is in the fragment's row iff cnt[c] >= 1 and 1000 * cnt[c] >= permille * n_coloured (64-bit).
// No orientation, no insert size: invariant under swapping the mates and under reversing either mate's slot order.
//   permille 1000, both mates with coloured slots: the AND of the mates' per-read rows (cnt_a[c] <= n_a and cnt_b[c] <= n_b, so cnt_a[c] + cnt_b[c] >= n_a + n_b
//                  forces both equalities); one mate without coloured slots: the other mate's row.  permille 0: the OR of the mates' rows.
//   mode FIN_PAIR_BOTH (1): the row is all zero unless BOTH mates have a coloured slot; the counts are reported either way.
//
// fin_pair_pseudo_kernel, a lane per fragment, the two adjacent records read together:
//   neither mate scanned (each kind 1, kind 2 or without pairs) -- mate a has na found slots in unitig ua, mate b nb in ub.  ca = (na > 0 and row(ua) non-empty)
//             ? na : 0, cb likewise; n_coloured = ca + cb, need = permille * n_coloured; word w: wa = row(ua)[w] if ca else 0, wb likewise;
//             pa = ca >= 1 && 1000 ca >= need, pb likewise, pab = ca + cb >= 1 (its threshold holds for every permille <= 1000);
//             out[w] = (wa & wb & M(pab)) | (wa & ~wb & M(pa)) | (wb & ~wa & M(pb)).  ua == ub is no special case.  W > 1: wave-cooperative, a ballot of the lanes on
//             this path, for each the wave loads both rows, lane i word i; one ballot each of wa != 0 and wb != 0 are the non-empty flags; lane i stores word i; a
//             wave sum is the popcount.  W = 1: a lane does its own fragment, coalesced as it is.
//   a mate scanned -- the wave takes such fragments one after the other with fin_colors.hip's register table (FinUnitigTable, entry i in lane i), SEEDED with (u, n) of a kind-1
//             partner, every entry with a second count: the slots that came from the first mate.  Either or both ranges are scanned through out_offs; the output
//             word is one ballot of the threshold test; n_coloured_first is a wave sum.
//   more than 64 distinct unitigs in the FRAGMENT -- the table is dropped, the fragment is rescanned: n_coloured from a lane per slot over both ranges plus the
//             seed, then for each word the ranges again plus the seed.  W + 1 rescans, exact.
// No LDS, no atomics, no global scratch; every output word has one writer.  A slot whose unitig number is at or above n_unitigs counts as absent.
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_wave.h"

#define FIN_PAIR_BLK 256u   // fragments per block: a lane per fragment

namespace {
typedef unsigned long long ull;

// read r as a mate: n found slots in unitig u (a kind-1 record), or the pair range [lo, hi) to scan (hi > lo), or nothing (n = 0, hi = lo = 0).
// SETS (here and below): the rows are keyed by set id (fin_wave.h: fin_row_key) -- bits = sets, n_unitigs = n_sets + 1, set_of and n_u the map and the index's unitigs
template <bool SETS>
__device__ __forceinline__ void pr_mate(const FinFastRec* frec, const uint64_t* out_offs, uint32_t r, uint32_t n_reads, uint32_t k, uint32_t n_unitigs, uint32_t& u,
                                        uint32_t& n, uint64_t& lo, uint64_t& hi, const uint32_t* set_of, uint32_t n_u) {
    const FinReadItem it = fin_read_item<false>(frec, out_offs, r, n_reads);
    if (it.kind == 1u && it.a.w != 0u && it.a.x < (SETS ? n_u : n_unitigs)) {
        (void)sgm_rec_walk(it.a, it.load_b(), k, [&](uint32_t, uint32_t from, uint32_t to) { n += to - from; });
        u = fin_row_key<SETS>(it.a.x, set_of, n_u);
    }
    if (it.scanned()) { lo = it.p_lo; hi = it.p_hi; }
}

// the closed form of two mates that lie in one unitig each: word w of the fragment's row from word w of the two rows (0 where the mate has no coloured slot)
__device__ __forceinline__ ull pr_closed(ull wa, ull wb, uint32_t ca, uint32_t cb, uint32_t permille, uint32_t mode) {
    const uint64_t need = (uint64_t)permille * (ca + cb);
    const bool pa = ca >= 1u && 1000ull * ca >= need, pb = cb >= 1u && 1000ull * cb >= need, pab = ca + cb >= 1u;
    if (mode == 1u && !(ca != 0u && cb != 0u)) return 0ull;
    return (wa & wb & (pab ? ~0ull : 0ull)) | (wa & ~wb & (pa ? ~0ull : 0ull)) | (wb & ~wa & (pb ? ~0ull : 0ull));
}

// slots [lo, hi) of one mate into the wave's table: its counts, and t_first -- the slots that came from the first mate -- beside them.  Wave-converged
template <bool SETS>
__device__ __forceinline__ void pr_table_scan(const int2* pairs, uint64_t lo, uint64_t hi, uint32_t n_unitigs, bool first, uint32_t& n_found, FinUnitigTable& tab,
                                              uint32_t& t_first, const uint32_t* set_of, uint32_t n_u) {
    fin_each_pair_row(pairs, lo, hi, [&](uint64_t, uint64_t, int2 p) {
        const uint32_t u = fin_row_key<SETS>((uint32_t)p.x, set_of, n_u);
        n_found += (uint32_t)__popcll(__ballot(u < n_unitigs));
        fin_each_distinct(u, u < n_unitigs, [&](int, uint32_t uc, ull m) {
            const uint32_t c = (uint32_t)__popcll(m);
            if (tab.add(uc, c) && first) t_first += c;   // (t_first is 0 in a lane without an entry)
        });
    });
}

// one fragment with a scanned mate: slots [alo, ahi) are the first mate's, [blo, bhi) the second's (either may be empty), the seed sn found slots in unitig su
// (sn = 0: none; sfirst: they are the first mate's).  Its row into out[0 .. W), its head returned in every lane.  Wave-converged
template <bool SETS>
__device__ __forceinline__ uint4 pr_scan(const int2* pairs, uint64_t alo, uint64_t ahi, uint64_t blo, uint64_t bhi, uint32_t su, uint32_t sn, bool sfirst, const ull* bits,
                                         uint32_t W, uint32_t n_unitigs, uint32_t permille, uint32_t mode, ull* out, const uint32_t* set_of, uint32_t n_u) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t n_found = sn, t_first = 0;
    FinUnitigTable tab;
    if (sn != 0u && tab.add(su, sn) && sfirst) t_first = sn;   // the seed is entry 0
    pr_table_scan<SETS>(pairs, alo, ahi, n_unitigs, true, n_found, tab, t_first, set_of, n_u);
    pr_table_scan<SETS>(pairs, blo, bhi, n_unitigs, false, n_found, tab, t_first, set_of, n_u);
    uint32_t n_colored = 0, n_first = 0, pc = 0;
    if (!tab.over) {
        const bool ne = tab.colored(bits, W);
        n_colored = fin_wave_sum(ne ? tab.t_cnt : 0u);
        n_first = fin_wave_sum(ne ? t_first : 0u);
        const bool keep = mode == 0u || (n_first != 0u && n_colored != n_first);
        const uint64_t need = (uint64_t)permille * n_colored;
        for (uint32_t w = 0; w < W; w++) pc += fin_row_word(tab.word_counts(bits, W, w), need, keep, out, w);
    } else {
        bool sne = false;                   // the seed's row: lane i looks at word i
        if (sn != 0u) sne = __ballot(lane < W && bits[(uint64_t)su * W + (lane < W ? lane : 0u)] != 0ull) != 0ull;
        const uint32_t sc = sne ? sn : 0u;
        n_first = fin_rescan_colored<SETS>(pairs, alo, ahi, bits, W, n_unitigs, set_of, n_u) + (sfirst ? sc : 0u);
        n_colored = n_first + fin_rescan_colored<SETS>(pairs, blo, bhi, bits, W, n_unitigs, set_of, n_u) + (sfirst ? 0u : sc);
        const bool keep = mode == 0u || (n_first != 0u && n_colored != n_first);
        const uint64_t need = (uint64_t)permille * n_colored;
        for (uint32_t w = 0; w < W; w++) {
            uint32_t cnt = fin_rescan_word<SETS>(pairs, alo, ahi, bits, W, n_unitigs, w, set_of, n_u) + fin_rescan_word<SETS>(pairs, blo, bhi, bits, W, n_unitigs, w, set_of, n_u);
            if (sn != 0u && ((bits[(uint64_t)su * W + w] >> lane) & 1ull)) cnt += sn;
            pc += fin_row_word(cnt, need, keep, out, w);
        }
    }
    return make_uint4(n_found, n_colored, pc, n_first);
}

// the body of fin_pair_pseudo_kernel and, with SETS, of fin_pair_pseudo_sets_kernel
template <bool SETS>
__device__ __forceinline__ void pr_body(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_frags, uint32_t k, const ull* bits, uint32_t W,
                                        uint32_t n_unitigs, uint32_t permille, uint32_t mode, ull* rows, uint4* heads, const uint32_t* set_of, uint32_t n_u) {
    const uint32_t f = blockIdx.x * FIN_PAIR_BLK + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t f0 = f - lane;           // the wave's first fragment
    uint32_t ua = 0, na = 0, ub = 0, nb = 0;   // a kind-1 mate's unitig and found slots
    uint64_t alo = 0, ahi = 0, blo = 0, bhi = 0;
    if (f < n_frags) {
        pr_mate<SETS>(frec, out_offs, 2u * f, 2u * n_frags, k, n_unitigs, ua, na, alo, ahi, set_of, n_u);
        pr_mate<SETS>(frec, out_offs, 2u * f + 1u, 2u * n_frags, k, n_unitigs, ub, nb, blo, bhi, set_of, n_u);
    }
    const bool scanned = ahi > alo || bhi > blo;
    uint4 mine = make_uint4(0u, 0u, 0u, 0u);
    // ---- neither mate scanned: the closed form over the two unitigs' rows ----
    if (W == 1u) {
        if (f < n_frags && !scanned) {
            const ull wa = na != 0u ? bits[ua] : 0ull, wb = nb != 0u ? bits[ub] : 0ull;
            const uint32_t ca = wa ? na : 0u, cb = wb ? nb : 0u;
            const ull o = pr_closed(wa, wb, ca, cb, permille, mode);
            rows[f] = o;
            mine = make_uint4(na + nb, ca + cb, (uint32_t)__popcll(o), ca);
        }
    } else {
        fin_each_lane(f < n_frags && !scanned, [&](int src) {
            const uint32_t uas = fin_bcast(ua, src), nas = fin_bcast(na, src), ubs = fin_bcast(ub, src), nbs = fin_bcast(nb, src);
            ull wa = 0ull, wb = 0ull;
            if (lane < W) {
                if (nas != 0u) wa = bits[(uint64_t)uas * W + lane];
                if (nbs != 0u) wb = bits[(uint64_t)ubs * W + lane];
            }
            const uint32_t ca = __ballot(wa != 0ull) ? nas : 0u, cb = __ballot(wb != 0ull) ? nbs : 0u;
            const ull o = pr_closed(wa, wb, ca, cb, permille, mode);
            if (lane < W) rows[(uint64_t)(f0 + (uint32_t)src) * W + lane] = o;
            const uint32_t pc = fin_wave_sum((uint32_t)__popcll(o));
            if ((int)lane == src) mine = make_uint4(nas + nbs, ca + cb, pc, ca);
        });
    }
    // ---- a mate scanned: the wave takes its lanes' fragments one after the other ----
    fin_each_lane(scanned, [&](int src) {
        const uint32_t nas = fin_bcast(na, src), nbs = fin_bcast(nb, src);   // (a scanned mate's n is 0: at most one of them is a seed)
        const uint32_t su = nas != 0u ? fin_bcast(ua, src) : fin_bcast(ub, src);
        const uint4 s = pr_scan<SETS>(pairs, fin_bcast64(alo, src), fin_bcast64(ahi, src), fin_bcast64(blo, src), fin_bcast64(bhi, src), su, nas + nbs, nas != 0u, bits, W,
                                      n_unitigs, permille, mode, rows + (uint64_t)(f0 + (uint32_t)src) * W, set_of, n_u);
        if ((int)lane == src) mine = s;
    });
    if (f < n_frags) heads[f] = mine;
}
}  // namespace

// rows[f][0 .. W) = fragment f's colour row, heads[f] = {n_found, n_coloured, popcount, n_coloured_first}; fragment f = reads 2f and 2f + 1.  frec null: the step
// left no records, every mate is scanned.
__global__ __launch_bounds__(256) void fin_pair_pseudo_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_frags, uint32_t k,
                                                              const ull* bits, uint32_t W, uint32_t n_unitigs, uint32_t permille, uint32_t mode, ull* rows, uint4* heads) {
    pr_body<false>(frec, out_offs, pairs, n_frags, k, bits, W, n_unitigs, permille, mode, rows, heads, nullptr, 0u);
}
// the same over a compact matrix: sets uint64[(n_sets + 1) * W] and set_of[n_unitigs]; every unitig number becomes its set id as it is loaded
__global__ __launch_bounds__(256) void fin_pair_pseudo_sets_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_frags, uint32_t k,
                                                                   const ull* sets, uint32_t W, uint32_t n_sets1, const uint32_t* set_of, uint32_t n_unitigs,
                                                                   uint32_t permille, uint32_t mode, ull* rows, uint4* heads) {
    pr_body<true>(frec, out_offs, pairs, n_frags, k, sets, W, n_sets1, permille, mode, rows, heads, set_of, n_unitigs);
}

// rows: uint64[n_frags * W]; heads: 16 bytes per fragment; out_offs and frec are the step's, over 2 n_frags reads.  mode: 0 any, 1 both
extern "C" int fin_launch_pseudoalign_paired(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_frags, uint32_t k, const void* bits, uint32_t W,
                                             uint32_t n_unitigs, uint32_t permille, uint32_t mode, void* rows, void* heads, hipStream_t stream) {
    const uint32_t nb = (n_frags + FIN_PAIR_BLK - 1u) / FIN_PAIR_BLK;
    if (nb == 0) return 0;
    hipLaunchKernelGGL(fin_pair_pseudo_kernel, dim3(nb), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs, n_frags, k, (const ull*)bits, W,
                       n_unitigs, permille, mode, (ull*)rows, (uint4*)heads);
    return (int)hipGetLastError();
}
// the same over a compact matrix: sets uint64[(n_sets + 1) * W], row 0 empty; set_of: uint32[n_unitigs], each <= n_sets
extern "C" int fin_launch_pseudoalign_paired_sets(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_frags, uint32_t k, const void* sets, uint32_t W,
                                                  uint32_t n_sets, const uint32_t* set_of, uint32_t n_unitigs, uint32_t permille, uint32_t mode, void* rows, void* heads,
                                                  hipStream_t stream) {
    const uint32_t nb = (n_frags + FIN_PAIR_BLK - 1u) / FIN_PAIR_BLK;
    if (nb == 0) return 0;
    hipLaunchKernelGGL(fin_pair_pseudo_sets_kernel, dim3(nb), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs, n_frags, k, (const ull*)sets, W,
                       n_sets + 1u, set_of, n_unitigs, permille, mode, (ull*)rows, (uint4*)heads);
    return (int)hipGetLastError();
}
