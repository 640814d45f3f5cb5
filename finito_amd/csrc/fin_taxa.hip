// fin_taxa.hip -- TAXONOMIC classification: a taxon per unitig from its colours, a taxon per read by Kraken's root-to-leaf rule, the tally of the reads per taxon
// and the clade counts (include/finito_amd.h: fin_taxonomy, fin_read_taxon, fin_batch_taxa, fin_batch_add_taxa).  The sibling of fin_classify.hip:
// there a unitig shared by several labels votes for nobody, here it votes for the deepest taxon that holds all of them, and a read is called as deep as its
// k-mers support.  The tree's two walks (fin_lca, fin_tax_covers) are fin_taxa.h's; the frame of the per-read kernel is fin_wave.h's.
//
// UNITIG LABELS.  label[u] = the LCA of color_taxon[c] over the set bits c of unitig u's colour row, FIN_NO_LABEL for an empty row.  Two shapes:
//   W == 1 -- a lane per unitig folds its one word.
//   W >= 2 -- a wave per unitig: lane w < W folds word w, a butterfly of fin_lca over the wave joins the words (lca is associative and commutative, "none" is
//             its identity; W <= 64).
// The root absorbs everything, so a fold stops there.
//
// PER READ.  c[t] = the found slots whose unitig's label is t; H = {t : c[t] > 0}; score(t) = the sum of c[a] over a in H on t's root path; S = max score;
// call = the LCA of every t in H with score(t) == S; clade(t) = the sum of c[x] over x in H at or below t.  While 1000 * clade(call) < confidence * nk or
// clade(call) < max(min_found, 1) the call moves to its parent, from the root to "unclassified".  All of it is invariant under reversing the slot order.
//   kind 1 -- one unitig, one label L, n found slots: score = clade = n at every level, the call is L or nothing.
//   kind 2 -- empty.
//   kind 0 -- the wave gathers the read's distinct labels with their counts into its register table (entry i in lane i), as fin_classify.hip does, in
//             label-ordered passes [floor, ceil).  ONE pass holds the whole read whenever it has at most 64 distinct labels.  Then everything is in registers:
//             a wave-uniform loop over the entries gives each lane its entry's score, a butterfly of fin_lca over the entries at S the call; with
//             m_i = lca(t_i, call) -- a node of the call's root path, and t_i is at or below a node x of that path iff m_i >= x -- clade(call) is the wave's sum of
//             the counts with m_i == call, and lifting steps from one m to the next lower one: between two of them the clade, and so the test, does not change.
//   more than 64 distinct labels: the passes go on as in cls_scan, each one's table complete for its label range.  A pass's scores are made by scanning the
//             read's pairs again (every distinct label of a row, against every entry); S and the tie LCA are folded over the passes.  Lifting scans the pairs
//             once per step: a lane per slot takes m = lca(label, call), the step counts the slots with m == call and finds the next lower m.  Exact for any number
//             of taxa; no LDS, no global scratch, no atomics, nothing allocated per read.
// A lane writes its read's result as one 16-byte store.
//
// TALLY.  direct[taxon] += 1 per classified read, direct[n_taxa] += 1 per other read: one atomic add per distinct slot per wave, as fin_cls_tally_kernel.
// CLADES.  clade[t] = the sum of direct over t's subtree, into a second buffer: a lane per taxon with a non-zero count adds it to itself and every ancestor with
// 64-bit atomic adds.  Lanes of a wave that reach the same node go on together from there: the first takes the others' counts, the others stop -- one atomic per
// distinct node per wave and level, and a wave adds to the root once.  Integer adds: exact in any order.
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_taxa.h"
#include "fin_wave.h"

#define FIN_TAX_BLK 256u

namespace {
typedef unsigned long long ull;

// fin_lca over the wave's 64 lanes, the result in every lane
__device__ __forceinline__ uint32_t tax_wave_lca(const uint32_t* parent, uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fin_lca(parent, v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}
// the LCA of the taxa of one word's set bits, colours 64 w .. 64 w + 63
__device__ __forceinline__ uint32_t tax_fold_word(ull word, const uint32_t* color_taxon, uint32_t w, const uint32_t* parent) {
    uint32_t acc = FIN_TAX_NONE;
    while (word && acc != 0u) {
        const uint32_t c = 64u * w + (uint32_t)(__ffsll((long long)word) - 1);
        word &= word - 1ull;
        acc = fin_lca(parent, acc, color_taxon[c]);
    }
    return acc;
}

// the read's result from its thresholds, once the call and its clade are known.  `fails`: the lifting test
__device__ __forceinline__ bool tax_fails(uint32_t clade, uint64_t nk, uint32_t min_found, uint32_t conf) {
    return 1000ull * (ull)clade < (ull)conf * nk || clade < max(min_found, 1u);
}

// slots [lo, hi) of the pair array are one read's: {taxon, score, clade, n_labelled}, the whole wave.  Wave-converged; every lane returns the same value
__device__ __forceinline__ uint4 tax_scan(const int2* pairs, uint64_t lo, uint64_t hi, const uint32_t* labels, uint32_t n_unitigs, const uint32_t* parent,
                                          uint32_t min_found, uint32_t conf) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nk = hi - lo;
    uint32_t n_labelled = 0, S = 0, call = FIN_TAX_NONE;
    uint32_t floor = 0;                     // this pass admits the labels in [floor, ceil)
    uint32_t t_lab = FIN_TAX_NONE, t_cnt = 0, n_ent = 0;
    bool whole = false;                     // the table holds the whole read: one pass gave nothing up
    for (;;) {
        uint32_t ceil = FIN_TAX_NONE;
        n_ent = 0; t_lab = FIN_TAX_NONE; t_cnt = 0;
        fin_each_pair_row(pairs, lo, hi, [&](uint64_t, uint64_t, int2 p) {
            const uint32_t u = (uint32_t)p.x;
            uint32_t L = FIN_TAX_NONE;
            if (u < n_unitigs) L = labels[u];
            if (floor == 0u) n_labelled += (uint32_t)__popcll(__ballot(L != FIN_TAX_NONE));
            ull rem = __ballot(L >= floor && L < ceil);
            while (rem) {                   // the row's distinct admitted labels (cls_scan's loop)
                const int src = __ffsll((long long)rem) - 1;
                const uint32_t Lc = fin_bcast(L, src);
                const ull m = __ballot(L == Lc);
                const uint32_t c = (uint32_t)__popcll(m);
                rem &= ~m;
                if (Lc >= ceil) continue;
                const bool mine = lane < n_ent && t_lab == Lc;
                if (__ballot(mine)) { if (mine) t_cnt += c; }
                else if (n_ent < 64u) {
                    if (lane == n_ent) { t_lab = Lc; t_cnt = c; }
                    n_ent++;
                } else {                    // full: the larger of Lc and the table's largest label waits for a later pass
                    const uint32_t M = (uint32_t)__builtin_amdgcn_readfirstlane((int)fin_wave_max(t_lab));
                    if (Lc < M) {
                        if (t_lab == M) { t_lab = Lc; t_cnt = c; }
                        ceil = M;
                    } else ceil = Lc;
                }
            }
        });
        const bool live = lane < n_ent;
        whole = floor == 0u && ceil == FIN_TAX_NONE;
        // the entries' scores
        uint32_t score = 0;
        if (whole) {
            for (uint32_t e = 0; e < n_ent; e++) {
                const uint32_t a = fin_bcast(t_lab, (int)e), ca = fin_bcast(t_cnt, (int)e);
                if (live && fin_tax_covers(parent, a, t_lab)) score += ca;
            }
        } else {
            fin_each_pair_row(pairs, lo, hi, [&](uint64_t, uint64_t, int2 p) {
                const uint32_t u = (uint32_t)p.x;
                uint32_t L = FIN_TAX_NONE;
                if (u < n_unitigs) L = labels[u];
                fin_each_distinct(L, L != FIN_TAX_NONE, [&](int, uint32_t Lc, ull m) {
                    if (live && fin_tax_covers(parent, Lc, t_lab)) score += (uint32_t)__popcll(m);
                });
            });
        }
        // fold into S and the LCA of the taxa at S
        const uint32_t s1 = fin_wave_max(live ? score : 0u);
        if (s1 != 0u && s1 >= S) {
            const uint32_t tie = tax_wave_lca(parent, live && score == s1 ? t_lab : FIN_TAX_NONE);
            call = s1 > S ? tie : fin_lca(parent, call, tie);
            S = s1;
        }
        if (ceil == FIN_TAX_NONE) break;
        floor = ceil;
    }
    if (call == FIN_TAX_NONE) return make_uint4(FIN_TAX_NONE, 0u, 0u, 0u);
    // lifting
    uint32_t clade = 0;
    if (whole) {
        const bool live = lane < n_ent;
        const uint32_t m = live ? fin_lca(parent, t_lab, call) : FIN_TAX_NONE;
        for (;;) {
            clade += fin_wave_sum(m == call ? t_cnt : 0u);
            if (!tax_fails(clade, nk, min_found, conf)) break;
            const uint32_t nxt = fin_wave_max(live && m < call ? m + 1u : 0u);   // the next node of the path at which the clade grows
            if (nxt == 0u) { call = FIN_TAX_NONE; break; }                     // none: the test fails all the way up, and at the root
            call = nxt - 1u;
        }
    } else {
        for (;;) {                          // (m is taken against the call of this step: every step counts its whole clade)
            uint32_t nxt = 0;
            clade = 0;
            fin_each_pair_row(pairs, lo, hi, [&](uint64_t, uint64_t, int2 p) {
                const uint32_t u = (uint32_t)p.x;
                uint32_t L = FIN_TAX_NONE;
                if (u < n_unitigs) L = labels[u];
                const uint32_t m = L != FIN_TAX_NONE ? fin_lca(parent, L, call) : FIN_TAX_NONE;
                clade += (uint32_t)__popcll(__ballot(m == call));
                nxt = max(nxt, L != FIN_TAX_NONE && m < call ? m + 1u : 0u);
            });
            if (!tax_fails(clade, nk, min_found, conf)) break;
            nxt = fin_wave_max(nxt);
            if (nxt == 0u) { call = FIN_TAX_NONE; break; }
            call = nxt - 1u;
        }
    }
    if (call == FIN_TAX_NONE) return make_uint4(FIN_TAX_NONE, S, n_labelled, n_labelled);
    return make_uint4(call, S, clade, n_labelled);
}
}  // namespace

// label[u] = the LCA of unitig u's colours' taxa.  W == 1: a lane per unitig
__global__ __launch_bounds__(256) void fin_tax_lca1_kernel(const ull* bits, uint32_t n_unitigs, const uint32_t* color_taxon, const uint32_t* parent, uint32_t* label) {
    const uint64_t u = (uint64_t)blockIdx.x * FIN_TAX_BLK + threadIdx.x;
    if (u < n_unitigs) label[u] = tax_fold_word(bits[u], color_taxon, 0u, parent);
}
// W >= 2: a wave per unitig, four unitigs per block
__global__ __launch_bounds__(256) void fin_tax_lcaw_kernel(const ull* bits, uint32_t W, uint32_t n_unitigs, const uint32_t* color_taxon, const uint32_t* parent,
                                                           uint32_t* label) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t u = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (u >= n_unitigs) return;             // (the whole wave)
    uint32_t acc = FIN_TAX_NONE;
    if (lane < W) acc = tax_fold_word(bits[u * W + lane], color_taxon, lane, parent);
    acc = tax_wave_lca(parent, acc);
    if (lane == 0u) label[u] = acc;
}

// out[r] = read r's taxon.  frec null: the step left no records, every read is scanned
__global__ __launch_bounds__(256) void fin_tax_read_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_reads, uint32_t k,
                                                           const uint32_t* labels, uint32_t n_unitigs, const uint32_t* parent, uint32_t min_found, uint32_t conf,
                                                           uint4* out) {
    const uint32_t r = blockIdx.x * FIN_TAX_BLK + threadIdx.x, lane = threadIdx.x & 63u;
    const FinReadItem it = fin_read_item<true>(frec, out_offs, r, n_reads);
    uint4 mine = make_uint4(FIN_TAX_NONE, 0u, 0u, 0u);
    if (it.kind == 1u && it.a.w != 0u) {
        uint32_t L = FIN_TAX_NONE, n = 0;
        if (it.a.x < n_unitigs) L = labels[it.a.x];
        (void)sgm_rec_walk(it.a, it.b, k, [&](uint32_t, uint32_t from, uint32_t to) { n += to - from; });
        if (L != FIN_TAX_NONE && n != 0u) {
            const uint64_t nk = out_offs[r + 1] - out_offs[r];
            mine = tax_fails(n, nk, min_found, conf) ? make_uint4(FIN_TAX_NONE, n, n, n) : make_uint4(L, n, n, n);
        }
    }
    fin_each_searched_read(it, [&](int src, uint64_t lo, uint64_t hi) {
        const uint4 s = tax_scan(pairs, lo, hi, labels, n_unitigs, parent, min_found, conf);
        if ((int)lane == src) mine = s;
    });
    if (r < n_reads) out[r] = mine;
}

// direct[taxon] += 1 for every classified read, direct[n_taxa] += 1 for every other; one atomic add per distinct slot per wave
__global__ __launch_bounds__(256) void fin_tax_tally_kernel(const uint4* rt, uint32_t n_reads, uint32_t n_taxa, ull* direct) {
    const uint32_t r = blockIdx.x * FIN_TAX_BLK + threadIdx.x, lane = threadIdx.x & 63u;
    const bool active = r < n_reads;
    uint32_t slot = 0xFFFFFFFFu;            // a lane beyond n_reads: no slot of the tally (n_taxa is at most 2^31)
    if (active) { const uint32_t t = rt[r].x; slot = t < n_taxa ? t : n_taxa; }
    fin_each_distinct(slot, active, [&](int src, uint32_t S, ull m) {
        if ((int)lane == src) atomicAdd(direct + S, (ull)__popcll(m));
    });
}

// clade[x] += direct[t] for every taxon t and every x on t's root path, t itself among them.  clade is zero before
__global__ __launch_bounds__(256) void fin_tax_clade_kernel(const ull* direct, const uint32_t* parent, uint32_t n_taxa, ull* clade) {
    const uint64_t t = (uint64_t)blockIdx.x * FIN_TAX_BLK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    ull d = t < n_taxa ? direct[t] : 0ull;
    uint32_t x = d != 0ull ? (uint32_t)t : 0xFFFFFFFFu;   // the node this lane adds to next; 0xFFFFFFFF: it has stopped
    while (__ballot(x != 0xFFFFFFFFu)) {
        fin_each_distinct(x, x != 0xFFFFFFFFu, [&](int src, uint32_t, ull m) {
            if (m & (m - 1ull)) {           // several lanes at one node: the first goes on with all their counts
                ull sum = 0;
                for (ull q = m; q; q &= q - 1ull) sum += fin_bcast64(d, __ffsll((long long)q) - 1);
                if ((m >> lane) & 1ull) { if ((int)lane == src) d = sum; else d = 0ull; }
            }
        });
        if (x != 0xFFFFFFFFu && d == 0ull) x = 0xFFFFFFFFu;   // (merged into another lane)
        if (x != 0xFFFFFFFFu) {
            atomicAdd(clade + x, d);
            x = x == 0u ? 0xFFFFFFFFu : parent[x];
        }
    }
}

extern "C" int fin_launch_taxa_labels(const uint64_t* bits, uint32_t W, uint32_t n_unitigs, const uint32_t* color_taxon, const uint32_t* parent, uint32_t* label,
                                      hipStream_t stream) {
    if (n_unitigs == 0) return 0;
    if (W == 1u) {
        const uint32_t nb = (uint32_t)(((uint64_t)n_unitigs + FIN_TAX_BLK - 1u) / FIN_TAX_BLK);
        hipLaunchKernelGGL(fin_tax_lca1_kernel, dim3(nb), dim3(256), 0, stream, (const ull*)bits, n_unitigs, color_taxon, parent, label);
    } else {
        const uint32_t nb = (uint32_t)(((uint64_t)n_unitigs + 3u) / 4u);
        hipLaunchKernelGGL(fin_tax_lcaw_kernel, dim3(nb), dim3(256), 0, stream, (const ull*)bits, W, n_unitigs, color_taxon, parent, label);
    }
    return (int)hipGetLastError();
}
extern "C" int fin_launch_taxa_reads(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, const uint32_t* labels,
                                     uint32_t n_unitigs, const uint32_t* parent, uint32_t min_found, uint32_t conf, void* out, hipStream_t stream) {
    const uint32_t nb = (n_reads + FIN_TAX_BLK - 1u) / FIN_TAX_BLK;
    if (nb == 0) return 0;
    hipLaunchKernelGGL(fin_tax_read_kernel, dim3(nb), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs, n_reads, k, labels, n_unitigs,
                       parent, min_found, conf, (uint4*)out);
    return (int)hipGetLastError();
}
extern "C" int fin_launch_taxa_tally(const void* rt, uint32_t n_reads, uint32_t n_taxa, uint64_t* direct, hipStream_t stream) {
    const uint32_t nb = (n_reads + FIN_TAX_BLK - 1u) / FIN_TAX_BLK;
    if (nb == 0) return 0;
    hipLaunchKernelGGL(fin_tax_tally_kernel, dim3(nb), dim3(256), 0, stream, (const uint4*)rt, n_reads, n_taxa, (ull*)direct);
    return (int)hipGetLastError();
}
extern "C" int fin_launch_taxa_clades(const uint64_t* direct, const uint32_t* parent, uint32_t n_taxa, uint64_t* clade, hipStream_t stream) {
    const uint32_t nb = (uint32_t)(((uint64_t)n_taxa + FIN_TAX_BLK - 1u) / FIN_TAX_BLK);
    if (nb == 0) return 0;
    hipLaunchKernelGGL(fin_tax_clade_kernel, dim3(nb), dim3(256), 0, stream, (const ull*)direct, parent, n_taxa, (ull*)clade);
    return (int)hipGetLastError();
}
