// fin_classify.hip -- a batch's results as one CLASS per read under a labelling of the unitigs, and the TALLY of the reads assigned to each label
// (include/finito_amd.h: fin_read_class, fin_labels, fin_batch_classify, fin_batch_add_classes).  The sibling of fin_readsum.hip: not "is this
// read in the reference" but "which of the reference's genomes, plasmids, bins or colours is it from".
//
// labels[u] is unitig u's label, below n_labels, or FIN_NO_LABEL: k-mers found there vote for nobody.  Over the read's output slots 0 .. nk - 1 every found
// slot with a labelled unitig counts c[label] += 1; the class is {label = argmax c (ties to the smaller label), n_best = c[label], n_second = the largest count
// among the other labels, n_labelled = the sum of c}, or {FIN_NO_LABEL, 0, 0, 0} when nothing was counted.  All four are the same when the slot order is
// reversed, so a record found on the reverse strand (meta bit 8) needs no special case.
//
// What is read (the frame is fin_wave.h's).  Where the step left records, a lane per read:
//   kind 1 -- the record and one label: the record lies in ONE unitig, the class is {labels[u], n, 0, n} with n = the sum of the stretches of sgm_rec_walk.
//   kind 2 -- the empty class.
//   kind 0 -- the wave scans the read's pairs, a row of 64 slots at a time, the next row loaded ahead.  Every found lane gathers its
//             unitig's label (u repeats along a segment: mostly one cache line); a loop over the row's DISTINCT labels (readlane of the first lane left, a ballot of the lanes with it, a popcount)
//             turns the row into (label, count) items, typically one or two.  The items go into a
//             table the wave keeps in its registers, entry i in lane i: a ballot finds the entry of a label, else lane n_ent takes the item.  At the read's end
//             two wave reductions give the class: the maximum of (count << 32) | ~label, then the largest count among the other entries.
//
// More than 64 distinct labels in one read: the read is scanned again, in label-ordered passes, and stays exact.  A pass admits the labels in [floor, ceil):
// floor is where the pass before stopped (0 at first), ceil starts unbounded.  When the table is full and a new label arrives, the larger of it and the table's
// largest label is given up -- dropped, or evicted in favour of the new one -- and ceil comes down to it: from then on the pass admits nothing at or above it.
// ceil only falls, so a label below the final ceil was never refused and never evicted: at the pass's end the table holds exactly the labels in [floor, ceil), each
// with its whole count.  The table is folded into the running {best, n_second}, floor = ceil, and the read is scanned again until a pass gives nothing up.  Every
// pass with a full table finishes at least 64 labels.  No LDS, no global scratch, no atomics, nothing allocated per read.
// A lane writes its read's class as one 16-byte store: every output word has one writer.
//
// The tally: read r is assigned to its label when n_best >= max(min_found, 1), 1000 * n_best >= min_permille * nk and n_best >= n_second + min_margin, in 64-bit
// arithmetic, nk from out_offs; reads[label] += 1, else reads[n_labels] += 1.  A lane per read; the adds are put together in the wave, one atomic add per
// distinct slot per wave (the same distinct-value loop): ten labels and millions of reads would otherwise queue on ten addresses.
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_wave.h"

#define FIN_CLS_BLK 256u        // reads per block: a lane per read
#define FIN_CLS_NONE 0xFFFFFFFFu   // FIN_NO_LABEL

namespace {
typedef unsigned long long ull;

// slots [lo, hi) of the pair array are one read's: its class {label, n_best, n_second, n_labelled}, the whole wave, a row of 64 slots at a time.
// Wave-converged; every lane returns the same value.  A unitig number at or above n_unitigs (the absent slot's 0xFFFFFFFF is one) has no label
__device__ __forceinline__ uint4 cls_scan(const int2* pairs, uint64_t lo, uint64_t hi, const uint32_t* labels, uint32_t n_unitigs) {
    const uint32_t lane = threadIdx.x & 63u;
    ull best = 0;                           // (count << 32) | ~label of the best label so far, over the passes done (0: none)
    uint32_t n_second = 0, n_labelled = 0;
    uint32_t floor = 0;                     // this pass admits the labels in [floor, ceil)
    for (;;) {
        uint32_t ceil = FIN_CLS_NONE;
        uint32_t n_ent = 0;                 // the table: entry i < n_ent in lane i
        uint32_t t_lab = FIN_CLS_NONE, t_cnt = 0;
        fin_each_pair_row(pairs, lo, hi, [&](uint64_t, uint64_t, int2 p) {
            const uint32_t u = (uint32_t)p.x;   // ((-1,-1) in a lane beyond the read's end)
            uint32_t L = FIN_CLS_NONE;
            if (u < n_unitigs) L = labels[u];
            if (floor == 0u) n_labelled += (uint32_t)__popcll(__ballot(L != FIN_CLS_NONE));   // (the first pass sees every slot)
            ull rem = __ballot(L >= floor && L < ceil);
            while (rem) {                   // the row's distinct admitted labels, one item each (its own text, not fin_each_distinct: profiles/r28/wave_frame.md)
                const int src = __ffsll((long long)rem) - 1;
                const uint32_t Lc = fin_bcast(L, src);
                const ull m = __ballot(L == Lc);
                const uint32_t c = (uint32_t)__popcll(m);
                rem &= ~m;
                if (Lc >= ceil) continue;   // (ceil came down inside this row)
                const bool mine = lane < n_ent && t_lab == Lc;
                if (__ballot(mine)) { if (mine) t_cnt += c; }
                else if (n_ent < 64u) {
                    if (lane == n_ent) { t_lab = Lc; t_cnt = c; }
                    n_ent++;
                } else {                    // full: the larger of Lc and the table's largest label waits for a later pass
                    const uint32_t M = (uint32_t)__builtin_amdgcn_readfirstlane((int)fin_wave_max(t_lab));   // (every lane holds it: kept wave-uniform for ceil)
                    if (Lc < M) {
                        if (t_lab == M) { t_lab = Lc; t_cnt = c; }
                        ceil = M;
                    } else ceil = Lc;
                }
            }
        });
        // fold the table into the running class: its best entry, the largest count among its others, and the loser of the two bests
        const bool live = lane < n_ent;
        const ull k1 = fin_wave_max64(live ? ((ull)t_cnt << 32) | (uint32_t)~t_lab : 0ull);
        const uint32_t s1 = fin_wave_max(live && t_lab != (uint32_t)~(uint32_t)k1 ? t_cnt : 0u);
        const ull loser = k1 > best ? best : k1;
        if (k1 > best) best = k1;
        n_second = max(n_second, max(s1, (uint32_t)(loser >> 32)));
        if (ceil == FIN_CLS_NONE) break;    // nothing was given up: every label is counted
        floor = ceil;
    }
    if (best == 0ull) return make_uint4(FIN_CLS_NONE, 0u, 0u, 0u);
    return make_uint4(~(uint32_t)best, (uint32_t)(best >> 32), n_second, n_labelled);
}
}  // namespace

// cls[r] = read r's class.  frec null: the step left no records, every read is scanned.
__global__ __launch_bounds__(256) void fin_cls_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_reads, uint32_t k,
                                                      const uint32_t* labels, uint32_t n_unitigs, uint4* cls) {
    const uint32_t r = blockIdx.x * FIN_CLS_BLK + threadIdx.x, lane = threadIdx.x & 63u;
    const FinReadItem it = fin_read_item<true>(frec, out_offs, r, n_reads);
    uint4 mine = make_uint4(FIN_CLS_NONE, 0u, 0u, 0u);
    if (it.kind == 1u && it.a.w != 0u) {
        uint32_t L = FIN_CLS_NONE, n = 0;
        if (it.a.x < n_unitigs) L = labels[it.a.x];
        (void)sgm_rec_walk(it.a, it.b, k, [&](uint32_t, uint32_t from, uint32_t to) { n += to - from; });
        if (L != FIN_CLS_NONE && n != 0u) mine = make_uint4(L, n, 0u, n);
    }
    fin_each_searched_read(it, [&](int src, uint64_t lo, uint64_t hi) {
        const uint4 s = cls_scan(pairs, lo, hi, labels, n_unitigs);
        if ((int)lane == src) mine = s;
    });
    if (r < n_reads) cls[r] = mine;
}

// reads[label] += 1 for every read assigned to its label, reads[n_labels] += 1 for every other read; one atomic add per distinct slot per wave
__global__ __launch_bounds__(256) void fin_cls_tally_kernel(const uint4* cls, const uint64_t* out_offs, uint32_t n_reads, uint32_t n_labels, uint32_t min_found,
                                                            uint32_t min_permille, uint32_t min_margin, ull* reads) {
    const uint32_t r = blockIdx.x * FIN_CLS_BLK + threadIdx.x, lane = threadIdx.x & 63u;
    const bool active = r < n_reads;
    uint32_t slot = 0xFFFFFFFFu;            // a lane beyond n_reads: no slot of the tally (n_labels is at most 2^31)
    if (active) {
        const uint4 c = cls[r];
        const uint64_t nb = c.y, nk = out_offs[r + 1] - out_offs[r];
        const bool ok = nb >= (uint64_t)max(min_found, 1u) && 1000ull * nb >= (uint64_t)min_permille * nk && nb >= (uint64_t)c.z + (uint64_t)min_margin;
        slot = ok && c.x < n_labels ? c.x : n_labels;
    }
    fin_each_distinct(slot, active, [&](int src, uint32_t S, ull m) {
        if ((int)lane == src) atomicAdd(reads + S, (ull)__popcll(m));
    });
}

extern "C" int fin_launch_classify(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, const uint32_t* labels,
                                   uint32_t n_unitigs, void* cls, hipStream_t stream) {
    const uint32_t nb = (n_reads + FIN_CLS_BLK - 1u) / FIN_CLS_BLK;
    if (nb == 0) return 0;
    hipLaunchKernelGGL(fin_cls_kernel, dim3(nb), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs, n_reads, k, labels, n_unitigs, (uint4*)cls);
    return (int)hipGetLastError();
}
extern "C" int fin_launch_class_tally(const void* cls, const uint64_t* out_offs, uint32_t n_reads, uint32_t n_labels, uint32_t min_found, uint32_t min_permille,
                                      uint32_t min_margin, uint64_t* reads, hipStream_t stream) {
    const uint32_t nb = (n_reads + FIN_CLS_BLK - 1u) / FIN_CLS_BLK;
    if (nb == 0) return 0;
    hipLaunchKernelGGL(fin_cls_tally_kernel, dim3(nb), dim3(256), 0, stream, (const uint4*)cls, out_offs, n_reads, n_labels, min_found, min_permille, min_margin,
                       (ull*)reads);
    return (int)hipGetLastError();
}
