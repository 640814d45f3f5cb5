// fin_wave.h -- the FRAME every per-read device consumer of a step's results stands in, stated once (device only; the record's meaning is fin_rec_walk.h's).
//
// What a consumer reads.  Where the step left records (kernel 4, merged strands, fast path on, text mode 1 or 2), a lane per read, by the record's kind:
//   kind 1 -- the 32-byte record alone: the found strand slots are [0, nk) minus at most eight gaps (fin_rec_gaps / sgm_rec_walk).  The read's pairs are never
//             touched -- in text mode 2 they do not exist.
//   kind 2 -- nothing: no slot of the read was found.
//   kind 0 -- the pipeline searched the read: its pairs are slots [out_offs[r], out_offs[r + 1]) of the pair array.  The wave takes its lanes' searched reads one
//             after the other and scans each a row of 64 slots at a time.
// Where the step left no records (frec null: forward-only search, kernels 0 / 2 / 3, fast path off, k > 63, text mode 0) every read is a kind-0 read.
// fin_hits.hip, fin_cover.hip, fin_depth.hip, fin_pileup.hip, fin_segments.hip, fin_readsum.hip, fin_classify.hip, fin_colors.hip and fin_paired.hip say only what is their own.
//
// Everything here is wave-converged unless it says "a lane": callers hand in lambdas that capture by reference; they inline, and what they capture stays in registers
// as long as nothing is indexed by a run-time count.
#pragma once
#include "fin_device.h"
#include "fin_rec_walk.h"

// ---- the wave ----
// lane src's value, for the whole wave
__device__ __forceinline__ uint32_t fin_bcast(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, src); }
__device__ __forceinline__ uint64_t fin_bcast64(uint64_t v, int src) { return ((uint64_t)fin_bcast((uint32_t)(v >> 32), src) << 32) | fin_bcast((uint32_t)v, src); }
// over the wave's 64 lanes, the result in every lane
__device__ __forceinline__ uint32_t fin_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}
__device__ __forceinline__ uint64_t fin_wave_sum64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, d);
    return v;
}
__device__ __forceinline__ uint32_t fin_wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}
__device__ __forceinline__ uint64_t fin_wave_max64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, d);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ double fin_wave_fmax(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d));
    return v;
}
// over a block of four waves, through lds_w[4]: the sum in every thread (one barrier; lds_w is not to be written again before the next one)
__device__ __forceinline__ uint32_t fin_block_sum4(uint32_t v, uint32_t* lds_w) {
    v = fin_wave_sum(v);
    if ((threadIdx.x & 63u) == 0u) lds_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return lds_w[0] + lds_w[1] + lds_w[2] + lds_w[3];
}
// ... the sum over the threads before this one (exclusive), and -- in *total, if not null -- over all of them
__device__ __forceinline__ uint32_t fin_block_exclusive4(uint32_t mine, uint32_t* lds_w, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)inc, d); if ((int)lane >= d) inc += y; }
    if (lane == 63u) lds_w[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; w++) before += lds_w[w];
    if (total) *total = lds_w[0] + lds_w[1] + lds_w[2] + lds_w[3];
    return before + inc - mine;
}
// f(src) for every lane src whose `pred` holds, ascending
template <class F>
__device__ __forceinline__ void fin_each_lane(bool pred, F&& f) {
    unsigned long long todo = __ballot(pred);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        f(src);
    }
}
// the distinct values v of the lanes with `valid`, one item each: f(src, vc, m) -- the first lane left, its value, the lanes that hold it.  A lane without
// `valid` must hold a value that no lane with it holds (an absent slot's 0xFFFFFFFF against "u < n_unitigs"): the loop's ballot does not look at `valid` again
template <class F>
__device__ __forceinline__ void fin_each_distinct(uint32_t v, bool valid, F&& f) {
    unsigned long long rem = __ballot(valid);
    while (rem) {
        const int src = __ffsll((long long)rem) - 1;
        const uint32_t vc = fin_bcast(v, src);
        const unsigned long long m = __ballot(v == vc);
        rem &= ~m;
        f(src, vc, m);
    }
}

// ---- a lane's read ----
// read r as its lane sees it.  kind 2 and nothing loaded for r >= n_reads; frec null: every read is kind 0.  a = {u, off0, meta, nk} where there is a record,
// b = the position words of a kind-1 record; slots [p_lo, p_hi) of the pair array for a kind-0 read.  LOAD_B: b is loaded here, right behind a, for every kind-1
// record -- the load is in flight across whatever the consumer does first (fin_sgm_kernel<true>: a block prefix with a barrier).  A consumer that wants b only
// for some kind-1 records (a check of u or nk comes first) takes fin_read_item<false> and calls load_b() there
struct FinReadItem {
    uint32_t kind;
    uint4 a, b;
    uint64_t p_lo, p_hi;
    const uint4* rec;
    __device__ __forceinline__ bool scanned() const { return kind == 0u && p_hi > p_lo; }
    __device__ __forceinline__ uint4 load_b() const { return rec[1]; }
};
template <bool LOAD_B>
__device__ __forceinline__ FinReadItem fin_read_item(const FinFastRec* frec, const uint64_t* out_offs, uint32_t r, uint32_t n_reads) {
    FinReadItem it = {2u, make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u), 0, 0, (const uint4*)(frec + r)};
    if (r < n_reads) {
        it.kind = 0u;
        if (frec) {
            it.a = it.rec[0];
            it.kind = it.a.z >> 16;
            if (LOAD_B && it.kind == 1u) it.b = it.rec[1];
        }
        if (it.kind == 0u) { it.p_lo = out_offs[r]; it.p_hi = out_offs[r + 1]; }
    }
    return it;
}
// the searched reads' pairs: the wave takes its lanes' reads one after the other -- f(src, lo, hi) with lane src's slot range
template <class F>
__device__ __forceinline__ void fin_each_searched_read(const FinReadItem& it, F&& f) {
    fin_each_lane(it.scanned(), [&](int src) { f(src, fin_bcast64(it.p_lo, src), fin_bcast64(it.p_hi, src)); });
}

// ---- a read's rows ----
// slots [lo, hi) of the pair array, a row of 64 at a time: f(base, j, p) with the row's first slot, the lane's slot and its pair -- (-1,-1) in a lane beyond hi.
// The row to come is loaded a row ahead: two loads in flight, the work on one row hides the other's latency
template <class F>
__device__ __forceinline__ void fin_each_pair_row(const int2* pairs, uint64_t lo, uint64_t hi, F&& f) {
    const uint32_t lane = threadIdx.x & 63u;
    int2 pn = make_int2(-1, -1);
    if (lo + lane < hi) pn = pairs[lo + lane];
    for (uint64_t base = lo; base < hi; base += 64u) {
        const uint64_t j = base + lane;
        const int2 p = pn;
        pn = make_int2(-1, -1);
        if (j + 64u < hi) pn = pairs[j + 64u];
        f(base, j, p);
    }
}

// ---- the head rule of a segment (fin_segments.hip states it) ----
// the last slot of the row before (0xFFFFFFFF: absent, or there is none) and its link: the two-slot history, wave-uniform
struct FinSegCarry { uint32_t pu = 0xFFFFFFFFu, poff = 0u; int plink = 0; };
// a lane's slot (u, off) of a row: its link to the slot before, and whether it is a segment head
__device__ __forceinline__ bool fin_seg_head(uint32_t u, uint32_t off, bool found, const FinSegCarry& c, int& link) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t up = (uint32_t)__shfl_up((int)u, 1), offp = (uint32_t)__shfl_up((int)off, 1);
    if (lane == 0u) { up = c.pu; offp = c.poff; }
    link = 0;
    if (found && u == up) link = off == offp + 1u ? 1 : off + 1u == offp ? -1 : 0;   // (u == up and found: the slot before is found too)
    int linkp = __shfl_up(link, 1);
    if (lane == 0u) linkp = c.plink;
    return found && (link == 0 || (linkp != 0 && linkp != link));
}
__device__ __forceinline__ void fin_seg_next_row(FinSegCarry& c, uint32_t u, uint32_t off, int link) {
    c.pu = fin_bcast(u, 63); c.poff = fin_bcast(off, 63);
    c.plink = __builtin_amdgcn_readlane(link, 63);
}

// ---- the wave's table of a read's distinct unitigs -- over a compact matrix, of its distinct SET IDS: counts are additive over the unitigs of one set --, for the
// colour rows (fin_colors.hip, fin_paired.hip): entry i < n_ent in lane i ----
struct FinUnitigTable {
    uint32_t n_ent = 0, t_u = 0, t_cnt = 0;
    bool over = false;                      // more than 64 distinct unitigs: the table is dropped, the caller rescans
    // c more slots in unitig uc; true in the lane that holds its entry.  Once `over`, nothing is added any more: a caller's distinct loop runs the row out idly
    __device__ __forceinline__ bool add(uint32_t uc, uint32_t c) {
        const uint32_t lane = threadIdx.x & 63u;
        if (over) return false;
        bool mine = lane < n_ent && t_u == uc;
        if (!__ballot(mine)) {
            if (n_ent == 64u) { over = true; return false; }
            mine = lane == n_ent;
            if (mine) t_u = uc;             // (t_cnt is 0 in a lane without an entry)
            n_ent++;
        }
        if (mine) t_cnt += c;
        return mine;
    }
    // a lane: its entry's unitig has a non-empty row
    __device__ __forceinline__ bool colored(const unsigned long long* bits, uint32_t W) const {
        const bool live = (threadIdx.x & 63u) < n_ent;
        const unsigned long long* row = bits + (uint64_t)t_u * W;   // (t_u = 0 in a lane without an entry: never read)
        bool ne = false;
        for (uint32_t w = 0; w < W; w++) if (live && row[w] != 0ull) ne = true;
        return ne;
    }
    // cnt[64 w + lane]: lane e gathers word w of its entry's row, a wave-uniform loop over the entries broadcasts word and count, lane b adds where bit b is set
    __device__ __forceinline__ uint32_t word_counts(const unsigned long long* bits, uint32_t W, uint32_t w) const {
        const uint32_t lane = threadIdx.x & 63u;
        const unsigned long long word = lane < n_ent ? bits[(uint64_t)t_u * W + w] : 0ull;
        uint32_t cnt = 0;
        for (uint32_t e = 0; e < n_ent; e++) {
            const unsigned long long we = fin_bcast64(word, (int)e);
            const uint32_t ce = fin_bcast(t_cnt, (int)e);
            if ((we >> lane) & 1ull) cnt += ce;
        }
        return cnt;
    }
};
// what keys the rows (fin_colors.hip, fin_paired.hip).  Over the dense matrix a unitig number is its own key.  Over a compact one (SETS; fin_colorsets.hip) it
// becomes its set id as it is loaded: bits = sets, n_unitigs = n_sets + 1, and a number at or above the index's n_u stays absent.  Set 0 is the empty row
template <bool SETS>
__device__ __forceinline__ uint32_t fin_row_key(uint32_t u, const uint32_t* set_of, uint32_t n_u) {
    if (SETS) return u < n_u ? set_of[u] : 0xFFFFFFFFu;
    return u;
}
// the rescans of a read whose table overflowed, a row at a time without looking ahead.  n_coloured of slots [lo, hi): a lane per slot looks at its unitig's row
template <bool SETS = false>
__device__ __forceinline__ uint32_t fin_rescan_colored(const int2* pairs, uint64_t lo, uint64_t hi, const unsigned long long* bits, uint32_t W, uint32_t n_unitigs,
                                                       const uint32_t* set_of = nullptr, uint32_t n_u = 0u) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t nc = 0;
    for (uint64_t base = lo; base < hi; base += 64u) {
        const uint64_t j = base + lane;
        uint32_t u = 0xFFFFFFFFu;
        if (j < hi) u = fin_row_key<SETS>((uint32_t)pairs[j].x, set_of, n_u);
        bool ne = false;
        if (u < n_unitigs) for (uint32_t w = 0; w < W; w++) if (bits[(uint64_t)u * W + w] != 0ull) ne = true;
        nc += (uint32_t)__popcll(__ballot(ne));
    }
    return nc;
}
// what slots [lo, hi) add to cnt[64 w + lane]: for each distinct unitig of a row its word w is broadcast, the lanes whose bit is set add the ballot's popcount
template <bool SETS = false>
__device__ __forceinline__ uint32_t fin_rescan_word(const int2* pairs, uint64_t lo, uint64_t hi, const unsigned long long* bits, uint32_t W, uint32_t n_unitigs, uint32_t w,
                                                    const uint32_t* set_of = nullptr, uint32_t n_u = 0u) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t cnt = 0;
    for (uint64_t base = lo; base < hi; base += 64u) {
        const uint64_t j = base + lane;
        uint32_t u = 0xFFFFFFFFu;
        if (j < hi) u = fin_row_key<SETS>((uint32_t)pairs[j].x, set_of, n_u);
        unsigned long long word = 0ull;
        if (u < n_unitigs) word = bits[(uint64_t)u * W + w];
        fin_each_distinct(u, u < n_unitigs, [&](int src, uint32_t, unsigned long long m) {
            if ((fin_bcast64(word, src) >> lane) & 1ull) cnt += (uint32_t)__popcll(m);
        });
    }
    return cnt;
}
// word w of a colour row from the counts: ONE BALLOT of the threshold test (all zero without `keep`), stored by one lane; returns its popcount
__device__ __forceinline__ uint32_t fin_row_word(uint32_t cnt, uint64_t need, bool keep, unsigned long long* out, uint32_t w) {
    const unsigned long long o = keep ? __ballot(cnt >= 1u && 1000ull * cnt >= need) : 0ull;
    if ((threadIdx.x & 63u) == 0u) out[w] = o;
    return (uint32_t)__popcll(o);
}
