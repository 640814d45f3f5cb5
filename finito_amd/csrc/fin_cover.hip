// fin_cover.hip -- a run's BREADTH over the unitig set: one bit per base of the concatenated unitig text, bit g set iff a query k-mer was found AT text position
// g = start(u) + off of its pair (u, off) (include/finito_amd.h: fin_cover, fin_batch_add_cover).  The sibling of fin_hits.hip: that one says how often a unitig
// was hit, this one which of its k-mers were.
//
// Position g is bit g & 63 of uint64 word g >> 6; the bitmap has (total_len + 63) / 64 words -- the geometry of safe[].  start(u) = ends_p[u].
//
// What is read (the frame is fin_wave.h's).  Where the step left records, a lane per read:
//   kind 1 -- slot sl of strand A is (u, off0 + sl) unless a gap of fin_rec_walk.h covers it.  Strand-slot order ascends in `off` whichever strand A is, so the
//             strand bit does not matter.  The lane walks the words that [g0, g0 + nk) touches and makes ONE mask per word -- the range's bits minus the gaps' --
//             and one OR: two or three for a 150-base read.
//   kind 0 -- the wave scans the read's pairs, a row of 64 slots at a time.  Neighbouring lanes are compared: a lane is a run head unless its
//             (u, off) continues the lane before it by one step in the run's direction.  Offsets ASCEND by one per slot for a read found on its forward strand
//             and DESCEND by one for a read found on its reverse strand (output slot i is strand slot nk - 1 - i): both merge.  A ballot gives each head its
//             run's length; only the head looks up start(u), and it issues one OR per (run, word) -- a run of at most 64 slots touches at most two words.
//             Absent slots set nothing.
// Where the step left no records the flat pair array is scanned the same way.
//
// ORs are 64-bit __hip_atomic_fetch_or, relaxed, agent scope, result unused.  OR is idempotent and commutative: the bitmap is exact whatever order the lanes
// arrive in, and the same run added twice changes nothing.
//
// Test before set (`probe`, option "cover_probe").  Past about 1x depth most words a read touches are already full.  With probe != 0 a lane first LOADS the word
// and skips the atomic when (w & m) == m.  This is exact: between two resets bits are only ever SET, so whatever a load returns -- a stale line, a value from
// before another lane's OR -- is a subset of the word's true content.  If the subset already holds every bit of m, so does the truth, and the OR would change
// nothing; if it does not, the lane ORs, possibly redundantly.  A stale view costs at most a redundant OR, never a lost one.  (A reset is ordered against the adds
// by the stream or by the events fin_cover_download waits for, like any other write.)
//
// Nothing here writes anything but the bitmap and the accumulator's flag word (bit 0: a step whose overflow list overran was offered -- nothing of it is set;
// bit 1: a unitig number outside the index, or a position at or beyond total_len, was met -- skipped).  Records, pairs and text are read only.  The kernels read
// the step's overflow counter themselves: no host synchronisation between step and add.  The device check is weaker than the host's (fin_records_cover
// refuses a k-mer that does not lie inside its own unitig): a record or pair whose offset runs past its unitig's end but stays inside the text sets bits in
// the neighbouring unitig without a flag.  The search kernels never produce such a place.
//
// fin_cover_count_kernel: covered[u] = popcount(bits[start(u) .. start(u + 1))), a thread per word, first and last word of every unitig masked; run on demand
// by fin_cover_download.
//
// Out of scope: partitioned indexes, fin_search_batch_multi, ORing across ranks (the caller ORs the downloaded bitmaps), per-position depth, the C++ mirror.
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_wave.h"

#define FIN_COVER_FLAT 4096u   // slots a wave scans in the flat form

namespace {
typedef unsigned long long ull;

__device__ __forceinline__ void cover_flag(uint32_t* flags, uint32_t bit) { (void)__hip_atomic_fetch_or(flags, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// bits[w] |= m.  The caller has checked that w is a word of the bitmap
__device__ __forceinline__ void cover_or(ull* bits, uint64_t w, ull m, bool probe) {
    if (m == 0ull) return;
    if (probe && (__hip_atomic_load(bits + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m) == m) return;   // (only ever set between resets: see the header)
    (void)__hip_atomic_fetch_or(bits + w, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the bits of text positions [a, b) that lie in the word that begins at position wb
__device__ __forceinline__ ull cover_word_mask(uint64_t wb, uint64_t a, uint64_t b) {
    const uint64_t lo = a > wb ? a : wb, hi = b < wb + 64u ? b : wb + 64u;
    if (lo >= hi) return 0ull;
    return (~0ull >> (64u - (uint32_t)(hi - lo))) << (uint32_t)(lo - wb);
}

// slots [lo, hi) of the pair array, a row of 64 at a time, the whole wave.  Wave-converged.
__device__ __forceinline__ void cover_scan(const int2* pairs, uint64_t lo, uint64_t hi, const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len, ull* bits,
                                           uint32_t* flags, bool probe) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = lo; base < hi; base += 64u) {
        const uint64_t j = base + lane;
        const bool act = j < hi;
        int2 p = make_int2(-1, -1);
        if (act) p = pairs[j];
        const uint32_t u = (uint32_t)p.x, off = (uint32_t)p.y;
        const bool found = act && u != 0xFFFFFFFFu;
        const uint32_t up = (uint32_t)__shfl_up((int)u, 1), offp = (uint32_t)__shfl_up((int)off, 1);
        const bool prev_found = __shfl_up((int)found, 1) != 0;
        const bool joins = found && prev_found && lane != 0u && u == up;
        const ull A = __ballot(act);
        const ull CU = __ballot(joins && off == offp + 1u), CD = __ballot(joins && off + 1u == offp);
        // a lane continues its predecessor's run only in that run's direction: one that steps up behind a lane that stepped down begins a run of its own
        const ull H = A & ~((CU & ~(CD << 1)) | (CD & ~(CU << 1)));   // run heads (absent slots are heads of nothing); bit 0 is set
        if (((H >> lane) & 1ull) && found) {
            const ull above = lane == 63u ? 0ull : (H >> (lane + 1u)) << (lane + 1u);
            const uint32_t end = above ? (uint32_t)__ffsll((long long)above) - 1u : (uint32_t)__popcll(A);
            const uint32_t n = end - lane;                                 // 1 .. 64
            const bool down = n > 1u && ((CD >> (lane + 1u)) & 1ull);
            if (u >= n_unitigs || (down && off < n - 1u)) cover_flag(flags, 2u);   // (the second cannot happen: the run's last offset would be negative)
            else {
                const uint64_t g0 = (uint64_t)ends_p[u] + (down ? off - (n - 1u) : off);
                uint64_t g1 = g0 + n;
                if (g1 > total_len) { cover_flag(flags, 2u); g1 = g0 < total_len ? total_len : g0; }   // (what lies inside the text is still set)
                if (g1 > g0) {
                    const uint64_t w = g0 >> 6;
                    cover_or(bits, w, cover_word_mask(w << 6, g0, g1), probe);
                    if (((g1 - 1u) >> 6) != w) cover_or(bits, w + 1u, cover_word_mask((w + 1u) << 6, g0, g1), probe);
                }
            }
        }
    }
}
}  // namespace

// A step that left records: a lane per read.  kind 1 -- the record's found ranges, a mask per word; kind 0 -- the wave scans the read's pairs
__global__ __launch_bounds__(256) void fin_cover_rec_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_reads, uint32_t k,
                                                            const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len, ull* bits, uint32_t* flags,
                                                            const uint32_t* ovf_count, uint32_t ovf_cap, uint32_t probe) {
    if (fin_step_withheld(ovf_count, ovf_cap, flags)) return;
    // the opening in this kernel's own text, not fin_read_item: a searched read's slot range is loaded BEHIND the record walk (profiles/r28/wave_frame.md, section 3)
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    uint32_t kind = 2u;
    uint64_t p_lo = 0, p_hi = 0;
    if (r < n_reads) {
        const uint4 a = ((const uint4*)(frec + r))[0];   // u, off0, meta, nk
        kind = a.z >> 16;
        if (kind == 1u && a.w != 0u) {
            const uint4 b = ((const uint4*)(frec + r))[1];
            const uint32_t nk = a.w;
            if (a.x >= n_unitigs) cover_flag(flags, 2u);
            else {
                const uint64_t g0 = (uint64_t)ends_p[a.x] + a.y;
                uint64_t g1 = g0 + nk;
                if (g1 > total_len) { cover_flag(flags, 2u); g1 = g0 < total_len ? total_len : g0; }   // (what lies inside the text is still set)
                for (uint64_t w = g0 >> 6; (w << 6) < g1; w++) {   // nk may reach 2^16 - 1: a loop over words, not a fixed count
                    ull m = cover_word_mask(w << 6, g0, g1);   // the range's bits, minus those of the gaps (fin_rec_walk.h; they do not depend on w)
                    fin_rec_gaps(nk, a.z & 0xFFu, b.x, b.y, b.z, b.w, k, [&](uint32_t lo, uint32_t hi_excl) { m &= ~cover_word_mask(w << 6, g0 + lo, g0 + hi_excl); });
                    cover_or(bits, w, m, probe != 0u);
                }
            }
        } else if (kind == 0u) { p_lo = out_offs[r]; p_hi = out_offs[r + 1]; }
    }
    fin_each_lane(kind == 0u && p_hi > p_lo, [&](int src) {
        cover_scan(pairs, fin_bcast64(p_lo, src), fin_bcast64(p_hi, src), ends_p, n_unitigs, total_len, bits, flags, probe != 0u);
    });
}

// A step that left no records: every slot of the pair array, FIN_COVER_FLAT consecutive slots per wave (runs then reach across reads, which a bitmap does not mind)
__global__ __launch_bounds__(256) void fin_cover_flat_kernel(const int2* pairs, uint64_t n_pairs, const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len,
                                                             ull* bits, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap, uint32_t probe) {
    if (fin_step_withheld(ovf_count, ovf_cap, flags)) return;
    const uint64_t n_spans = (n_pairs + FIN_COVER_FLAT - 1u) / FIN_COVER_FLAT;
    for (uint64_t s = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); s < n_spans; s += (uint64_t)gridDim.x * 4u) {
        const uint64_t lo = s * FIN_COVER_FLAT, hi = lo + FIN_COVER_FLAT < n_pairs ? lo + FIN_COVER_FLAT : n_pairs;
        cover_scan(pairs, lo, hi, ends_p, n_unitigs, total_len, bits, flags, probe != 0u);
    }
}

// covered[u] += the set bits of unitig u: a thread per bitmap word.  The word's first position is looked up in ends_p (the unitig u with
// ends_p[u] <= 64 w < ends_p[u + 1]); from there every unitig that begins inside the word takes its share -- several of them when unitigs are shorter than a
// word.  A wave whose 64 words all lie inside one unitig adds once.  covered[] is zeroed by the caller.
__global__ __launch_bounds__(256) void fin_cover_count_kernel(const ull* bits, uint64_t n_words, const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len, ull* covered) {
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool act = w < n_words;
    const ull x = act ? bits[w] : 0ull;
    const uint64_t wb = w << 6;
    uint32_t u = 0;
    bool inside = false;   // the whole word lies in unitig u
    if (act) {
        uint32_t lo = 0, hi = n_unitigs;   // the last u in [0, n_unitigs) with ends_p[u] <= wb (ends_p[0] = 0)
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if ((uint64_t)ends_p[mid] <= wb) lo = mid; else hi = mid; }
        u = lo;
        inside = (uint64_t)ends_p[u + 1] >= wb + 64u;
    }
    // one unitig for the whole wave: one add
    const uint32_t u0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)u);
    if (__ballot(act && !(inside && u == u0)) == 0ull) {
        const uint32_t c = fin_wave_sum((uint32_t)__popcll(x));
        if ((threadIdx.x & 63u) == 0u && c) (void)__hip_atomic_fetch_add(covered + u0, (ull)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if (!act || x == 0ull) return;
    const uint64_t we = wb + 64u < total_len ? wb + 64u : total_len;
    for (; u < n_unitigs; u++) {
        const uint64_t s = ends_p[u], e = ends_p[u + 1];
        if (s >= we) break;
        const uint32_t c = (uint32_t)__popcll(x & cover_word_mask(wb, s, e));
        if (c) (void)__hip_atomic_fetch_add(covered + u, (ull)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// bits: uint64[(total_len + 63) / 64]; flags: one u32 (bit 0: a step without results was offered, bit 1: a unitig number or position outside the index).
// frec null: the flat form.  ovf_count (may be null) / ovf_cap: the step's overflow list, as batch_overrun_check reads it.  probe: option "cover_probe"
extern "C" int fin_launch_cover_add(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint64_t n_pairs, uint32_t k, const uint32_t* ends_p,
                                    uint32_t n_unitigs, uint64_t total_len, void* bits, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap, uint32_t probe,
                                    hipStream_t stream) {
    if (n_reads == 0 || n_unitigs == 0 || total_len == 0) return 0;
    if (frec) {
        hipLaunchKernelGGL(fin_cover_rec_kernel, dim3((n_reads + 255u) / 256u), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs, n_reads, k,
                           ends_p, n_unitigs, total_len, (ull*)bits, flags, ovf_count, ovf_cap, probe);
    } else {
        if (n_pairs == 0) return 0;
        const uint64_t want = ((n_pairs + FIN_COVER_FLAT - 1u) / FIN_COVER_FLAT + 3u) / 4u;
        hipLaunchKernelGGL(fin_cover_flat_kernel, dim3((uint32_t)(want < 65536u ? want : 65536u)), dim3(256), 0, stream, (const int2*)pairs, n_pairs, ends_p, n_unitigs,
                           total_len, (ull*)bits, flags, ovf_count, ovf_cap, probe);
    }
    return (int)hipGetLastError();
}

// covered: uint64[n_unitigs], zeroed on `stream` here
extern "C" int fin_launch_cover_count(const void* bits, const uint32_t* ends_p, uint32_t n_unitigs, uint64_t total_len, void* covered, hipStream_t stream) {
    if (n_unitigs == 0) return 0;
    hipError_t e = hipMemsetAsync(covered, 0, (size_t)n_unitigs * 8, stream);
    if (e != hipSuccess) return (int)e;
    const uint64_t n_words = (total_len + 63u) / 64u;
    if (n_words == 0) return 0;
    hipLaunchKernelGGL(fin_cover_count_kernel, dim3((uint32_t)((n_words + 255u) / 256u)), dim3(256), 0, stream, (const ull*)bits, n_words, ends_p, n_unitigs, total_len,
                       (ull*)covered);
    return (int)hipGetLastError();
}
