// fin_fragments.hip -- the FRAGMENT GEOMETRY of paired reads: for fragment f = reads 2f (first mate) and 2f + 1 (second mate) of a finished step, where its mates
// lie, which way they face and how long the fragment is; summed over a run, the insert-size histogram and the six class counters
// (include/finito_amd.h: FRAGMENT GEOMETRY states the definition, fin_fragment, fin_fragments, fin_batch_add_fragments, fin_batch_fragments).
// fin_paired.hip pools a fragment's slots into one bag; this file is the part of a fragment that the bag forgets.
//
// A mate is PLACED by the pileup's rules 1 and 2 (fin_pileup.hip), no mismatch rule and no bases: straight -- at least two found slots, one unitig, one diagonal --
// and strand A at offsets [s0, s0 + L) inside its unitig, L = nk + k - 1.  All arithmetic is in integers.
//
// fin_fragments_kernel, a lane per fragment, the two adjacent records read together (the frame is fin_wave.h's):
//   a kind-1 mate -- the record alone: u, s0 = off0, direction (meta bit 8), nk; its bounds against ends_p first (outside: flag bit 1, as fin_pileup_add_kernel), then
//             the position words only for "at least two found slots" (sgm_rec_walk).  Pairs are never touched.
//   a scanned mate -- the wave takes such mates one after the other, the first mates before the second ones: pass 1 of fin_pileup.hip's pile_searched, restated -- the
//             first found slot's u, dF and dR, the found count, a ballot per row and diagonal (fin_each_pair_row).  No bases, no text.
//   frec null (k > 63, fast path off) -- every mate is scanned.
// Class, length and the 16-byte fin_fragment are lane-local once both mates are known.
//
// The accumulator: a block counts its inward fragments in an LDS table of n_bins uint32 (16 KB at most: eight blocks a CU fit beside each other, so LDS does not
// cap the 32 waves) -- zeroed, barrier, one LDS atomic per inward fragment, barrier -- and flushes the non-zero bins with relaxed, agent-scope 64-bit adds, result
// unused.  The six class counters and len_sum are summed over the wave first, then over the block in LDS, one global add each.  Integer adds commute: the result is
// exact whatever order the blocks arrive in, and a run added twice counts twice.  A withheld step returns before the first barrier, the whole block alike.
// No waiting, no floating point, no scratch.  frags null: nothing is stored per fragment; hist null: nothing is accumulated.
//
// Out of scope: a proper-pair filter inside fin_pair_pseudo_kernel, fragments that bridge unitigs, strand-specific library types, partitioned indexes,
// fin_search_batch_multi / dist.py, the C++ mirror.
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_wave.h"

#define FIN_FRAG_BLK 256u        // fragments per block: a lane per fragment
#define FIN_FRAG_LDS_BINS 4096u  // the most bins an accumulator has (FIN_FRAG_MAX_BINS)

namespace {
typedef unsigned long long ull;

// where a mate lies: strand A at offsets [s0, s0 + L) of unitig u; rev: strand A is the read's reverse complement
struct FgMate { uint32_t u, s0, L; bool placed, rev; };

__device__ __forceinline__ void fg_flag(uint32_t* flags, uint32_t bit) { (void)__hip_atomic_fetch_or(flags, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a kind-1 mate, a lane: the record alone
__device__ __forceinline__ FgMate fg_record(const FinReadItem& it, uint32_t k, const uint32_t* ends_p, uint32_t n_unitigs, uint32_t* flags) {
    FgMate m = {0xFFFFFFFFu, 0u, 0u, false, false};
    const uint4 a = it.a;
    if (a.w == 0u) return m;
    const uint32_t L = a.w + k - 1u;
    // u and the extent against the unitig's bounds before anything is counted.  (fin_pileup.hip also holds uend against total_len, because it goes on to index the
    // text and its per-position arrays with it; nothing here is indexed by a text position, so ends_p -- the replica's own table, n_unitigs + 1 entries -- is all
    // the rule needs)
    uint64_t ustart = 0, uend = 0;
    if (a.x < n_unitigs) { ustart = ends_p[a.x]; uend = ends_p[a.x + 1u]; }
    if (a.x >= n_unitigs || ustart + a.y + L > uend) { fg_flag(flags, 2u); return m; }
    uint32_t n_found = 0;
    (void)sgm_rec_walk(a, it.load_b(), k, [&](uint32_t, uint32_t from, uint32_t to) { n_found += to - from; });
    if (n_found < 2u) return m;
    m.u = a.x; m.s0 = a.y; m.L = L; m.placed = true; m.rev = (a.z >> 8) & 1u;
    return m;
}

// a scanned mate, the whole wave: slots [lo, hi) of the pair array.  Pass 1 of pile_searched (fin_pileup.hip) and its placement, nothing else.  Wave-converged;
// the result is the same in every lane
__device__ __forceinline__ FgMate fg_searched(const int2* pairs, uint64_t lo, uint64_t hi, uint32_t k, const uint32_t* ends_p, uint32_t n_unitigs, uint32_t* flags) {
    FgMate m = {0xFFFFFFFFu, 0u, 0u, false, false};
    uint32_t n_found = 0, u0 = 0;
    int32_t dF = 0, dR = 0;
    bool okF = true, okR = true, outside = false;
    fin_each_pair_row(pairs, lo, hi, [&](uint64_t, uint64_t j, int2 p) {
        const uint32_t u = (uint32_t)p.x;
        const bool found = u != 0xFFFFFFFFu;           // (a lane beyond hi holds (-1,-1))
        const ull F = __ballot(found);
        if (F == 0ull) return;
        const int32_t i = (int32_t)(uint32_t)(j - lo), f = p.y - i, r = p.y + i;
        if (n_found == 0u) {
            const int src = __ffsll((long long)F) - 1;
            u0 = fin_bcast(u, src); dF = (int32_t)fin_bcast((uint32_t)f, src); dR = (int32_t)fin_bcast((uint32_t)r, src);
        }
        n_found += (uint32_t)__popcll(F);
        if (__ballot(found && u >= n_unitigs)) outside = true;
        if (__ballot(found && (u != u0 || f != dF))) okF = false;
        if (__ballot(found && (u != u0 || r != dR))) okR = false;
    });
    if (outside) { if ((threadIdx.x & 63u) == 0u) fg_flag(flags, 2u); return m; }
    if (n_found < 2u || okF == okR) return m;          // (with two found slots both diagonals cannot hold; neither: a mosaic, an indel, a repeated pair)
    const uint32_t nk = (uint32_t)(hi - lo), L = nk + k - 1u;
    const bool rev = okR;
    const int64_t s0 = rev ? (int64_t)dR - (int64_t)nk + 1 : (int64_t)dF;
    const uint64_t ustart = ends_p[u0], uend = ends_p[u0 + 1u];   // (u0 < n_unitigs: not outside)
    if (s0 < 0 || ustart + (uint64_t)s0 + L > uend) return m;     // hangs over an end of its unitig
    m.u = u0; m.s0 = (uint32_t)s0; m.L = L; m.placed = true; m.rev = rev;
    return m;
}

// the fragment of two mates (include/finito_amd.h: the classes), a lane: {u, start, length, cls}
__device__ __forceinline__ uint4 fg_combine(const FgMate& a, const FgMate& b) {
    const uint32_t bits = (a.placed && a.rev ? 0x100u : 0u) | (b.placed && b.rev ? 0x200u : 0u) | (a.placed ? 0x400u : 0u) | (b.placed ? 0x800u : 0u);
    if (!a.placed && !b.placed) return make_uint4(0xFFFFFFFFu, 0u, 0u, bits);
    if (a.placed != b.placed) { const FgMate& m = a.placed ? a : b; return make_uint4(m.u, m.s0, m.L, 1u | bits); }
    if (a.u != b.u) return make_uint4(0xFFFFFFFFu, 0u, 0u, 2u | bits);
    const uint64_t ea = (uint64_t)a.s0 + a.L, eb = (uint64_t)b.s0 + b.L;   // (both inside one unitig: below 2^32)
    const uint32_t start = min(a.s0, b.s0), length = (uint32_t)(max(ea, eb) - start);
    uint32_t cls = 3u;
    if (a.rev != b.rev) {
        const bool a_fwd = !a.rev;
        const uint32_t sF = a_fwd ? a.s0 : b.s0, sR = a_fwd ? b.s0 : a.s0;
        const uint64_t eF = a_fwd ? ea : eb, eR = a_fwd ? eb : ea;
        cls = sF <= sR && eF <= eR ? 5u : 4u;
    }
    return make_uint4(a.u, start, length, cls | bits);
}
}  // namespace

// frags[f] = fragment f (may be null); hist[n_bins], counters[7] (may be null together): += the run's inward lengths, its classes and len_sum.  flags: the
// accumulator's flag word, or a word of the batch's own when only frags are wanted.  frec null: every mate is scanned
__global__ __launch_bounds__(256) void fin_fragments_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_frags, uint32_t k,
                                                            const uint32_t* ends_p, uint32_t n_unitigs, uint32_t n_bins, uint32_t bin_width, uint4* frags, ull* hist,
                                                            ull* counters, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap) {
    __shared__ uint32_t lds_hist[FIN_FRAG_LDS_BINS];
    __shared__ ull lds_cnt[8];
    if (fin_step_withheld(ovf_count, ovf_cap, flags)) return;
    const uint32_t f = blockIdx.x * FIN_FRAG_BLK + threadIdx.x, lane = threadIdx.x & 63u;
    if (hist) {
        for (uint32_t b = threadIdx.x; b < n_bins; b += FIN_FRAG_BLK) lds_hist[b] = 0u;
        if (threadIdx.x < 8u) lds_cnt[threadIdx.x] = 0ull;
    }
    const uint32_t n_reads = 2u * n_frags, r0 = f < n_frags ? 2u * f : n_reads;   // (a lane beyond the last fragment holds two kind-2 items)
    const FinReadItem ia = fin_read_item<false>(frec, out_offs, r0, n_reads);
    const FinReadItem ib = fin_read_item<false>(frec, out_offs, r0 < n_reads ? r0 + 1u : n_reads, n_reads);
    FgMate ma = {0xFFFFFFFFu, 0u, 0u, false, false}, mb = ma;
    if (ia.kind == 1u) ma = fg_record(ia, k, ends_p, n_unitigs, flags);
    if (ib.kind == 1u) mb = fg_record(ib, k, ends_p, n_unitigs, flags);
    fin_each_searched_read(ia, [&](int src, uint64_t lo, uint64_t hi) {
        const FgMate m = fg_searched(pairs, lo, hi, k, ends_p, n_unitigs, flags);
        if ((int)lane == src) ma = m;
    });
    fin_each_searched_read(ib, [&](int src, uint64_t lo, uint64_t hi) {
        const FgMate m = fg_searched(pairs, lo, hi, k, ends_p, n_unitigs, flags);
        if ((int)lane == src) mb = m;
    });
    const uint4 fr = fg_combine(ma, mb);
    const uint32_t cls = f < n_frags ? fr.w & 0xFFu : 6u;   // 6: no fragment
    if (frags && f < n_frags) frags[f] = fr;
    if (!hist) return;                                      // (the same in every thread)
    __syncthreads();
    const bool inward = cls == 5u;
    if (inward) {
        const uint32_t q = fr.z / bin_width;
        (void)__hip_atomic_fetch_add(lds_hist + (q < n_bins - 1u ? q : n_bins - 1u), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // the counters: a wave's fragments by class and its inward lengths, one LDS add each
#pragma unroll
    for (uint32_t c = 0; c < 6u; c++) {
        const ull n = (ull)__popcll(__ballot(cls == c));
        if (n && lane == 0u) (void)__hip_atomic_fetch_add(lds_cnt + c, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    const ull len_sum = fin_wave_sum64(inward ? (ull)fr.z : 0ull);
    if (len_sum && lane == 0u) (void)__hip_atomic_fetch_add(lds_cnt + 6, len_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < n_bins; b += FIN_FRAG_BLK) {
        const uint32_t v = lds_hist[b];
        if (v) (void)__hip_atomic_fetch_add(hist + b, (ull)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x < 7u && lds_cnt[threadIdx.x]) (void)__hip_atomic_fetch_add(counters + threadIdx.x, lds_cnt[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// frags: 16 bytes per fragment, or null; hist: uint64[n_bins] and counters: uint64[7], or both null; flags: one u32 (never null).  out_offs and frec are the
// step's, over 2 n_frags reads; frec null: every mate is scanned.  ovf_count (may be null) / ovf_cap as fin_launch_depth_add
extern "C" int fin_launch_fragments(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_frags, uint32_t k, const uint32_t* ends_p, uint32_t n_unitigs,
                                    uint32_t n_bins, uint32_t bin_width, void* frags, void* hist, void* counters, uint32_t* flags, const uint32_t* ovf_count,
                                    uint32_t ovf_cap, hipStream_t stream) {
    if (n_frags == 0) return 0;
    if (k == 0 || !flags || (hist && (!counters || n_bins == 0 || n_bins > FIN_FRAG_LDS_BINS || bin_width == 0)) || n_frags > 0x7FFFFFFFu) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fin_fragments_kernel, dim3((n_frags + FIN_FRAG_BLK - 1u) / FIN_FRAG_BLK), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs,
                       n_frags, k, ends_p, n_unitigs, n_bins, bin_width, (uint4*)frags, (ull*)hist, (ull*)counters, flags, ovf_count, ovf_cap);
    return (int)hipGetLastError();
}
