// fin_hits.hip -- a run's PROFILE over the unitig set: counts[u] += the query k-mers of the most recent step that were found in unitig u
// (include/finito_amd.h: fin_hits, fin_batch_add_hits).
//
// Nothing per k-mer leaves the device and, for the reads the pair pre-pass's fast path finished, nothing per k-mer is even read: such a read is a 32-byte
// record (FinFastRec) and its share of the profile is ONE number for ONE unitig -- nk minus the slots a disagreeing position covers, nk minus the summed
// gaps of fin_rec_walk.h, worked out by one lane.  The other reads' pairs are scanned where the step left them: consecutive slots with the
// same unitig are one run, and a run is one add.  A step that left no records (forward-only search, the other kernels, fast path off, text mode 0) is the
// flat pair array scanned end to end; runs then reach across reads, which a count does not mind.
//
// Adds are 64-bit integer atomics, relaxed, device scope: exact whatever order they arrive in.  `combine` (option "hits_combine") says how much is summed
// inside a wave before an add goes to memory:
//   records: up to `combine` rounds in which the first lane still holding a number takes over the numbers of every lane with the same unitig (one wave
//            sum, one add); whoever is left adds alone.  On an index of three unitigs three rounds empty the wave; on chr1 (10^6 unitigs and more, a
//            wave's 64 reads in 64 of them) the rounds find nothing to merge and cost a few wave sums.
//   pairs:   the slots of a wave's 64 that lie in the unitig of the last found one are counted (a ballot) and held back, and joined by those of its next 64
//            slots while the unitig stays the same: a read inside one unitig, absent stretches and all, or a wave's whole stretch of a one-unitig index,
//            is one add.  (An add that goes to memory holds up the wave's next load -- they share a counter --, so adds saved are latency saved.)
//   0:       every record lane and every run head of a 64-slot row adds by itself.
// Nothing here writes anything but counts[] and the accumulator's flag word; the records and the pairs are read only.
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_wave.h"

#define FIN_HITS_FLAT 4096u   // slots a wave scans in the flat form (64 rows: the held-back run pays off)

namespace {
typedef unsigned long long ull;

__device__ __forceinline__ void hits_add(ull* counts, uint32_t n_unitigs, uint32_t* flags, uint32_t u, ull n) {
    if (n == 0ull) return;
    if (u < n_unitigs) (void)__hip_atomic_fetch_add(counts + u, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else (void)__hip_atomic_fetch_or(flags, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a unitig the index does not have: never written, reported by fin_hits_download)
}

// The run a wave holds back between rows of pairs: wave-uniform
struct HitsCarry { uint32_t u; ull n; };

// slots [lo, hi) of the pair array, a row of 64 at a time, the whole wave.  Wave-converged.
__device__ __forceinline__ void hits_scan(const int2* pairs, uint64_t lo, uint64_t hi, ull* counts, uint32_t n_unitigs, uint32_t* flags, bool combine, HitsCarry& c) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = lo; base < hi; base += 64u) {
        const uint64_t j = base + lane;
        const bool act = j < hi;
        const uint32_t u = act ? (uint32_t)pairs[j].x : 0xFFFFFFFFu;   // (absent slots are -1: a run like any other that nobody adds)
        const uint32_t up = (uint32_t)__shfl_up((int)u, 1);
        const ull A = __ballot(act);
        const ull H = __ballot(act && (lane == 0u || u != up));        // run heads; bit 0 is set
        // the run of a head lane ends in front of the next head, or with the row's last slot
        const ull above = lane == 63u ? 0ull : (H >> (lane + 1u)) << (lane + 1u);
        const uint32_t end = above ? (uint32_t)__ffsll((long long)above) - 1u : (uint32_t)__popcll(A);
        const ull n = (ull)(end - lane);
        const bool head = (H >> lane) & 1ull;
        if (!combine) { if (head && u != 0xFFFFFFFFu) hits_add(counts, n_unitigs, flags, u, n); continue; }
        // the unitig of the row's last FOUND run is the one held back; every slot of the row in that unitig joins it (a read with a few absent stretches
        // is u, -1, u, -1, u: one add; a row of absent slots leaves what is held back alone), and so does what was held back so far when it is in that
        // unitig too -- else that goes to memory now
        const ull F = __ballot(head && u != 0xFFFFFFFFu);
        if (F == 0ull) continue;
        const uint32_t last = 63u - (uint32_t)__clzll((long long)F);
        const uint32_t ul = fin_bcast(u, (int)last);
        const uint32_t s = (uint32_t)__popcll(__ballot(act && u == ul));
        if (head && u != ul && u != 0xFFFFFFFFu) hits_add(counts, n_unitigs, flags, u, n);
        if (c.n && c.u != ul) { if (lane == 0u) hits_add(counts, n_unitigs, flags, c.u, c.n); c.n = 0ull; }
        c.u = ul; c.n += (ull)s;
    }
}
__device__ __forceinline__ void hits_flush(ull* counts, uint32_t n_unitigs, uint32_t* flags, HitsCarry& c) {
    if ((threadIdx.x & 63u) == 0u && c.n) hits_add(counts, n_unitigs, flags, c.u, c.n);
    c.n = 0ull;
}
}  // namespace

// A step that left records: a lane per read (fin_wave.h).  kind 1 -- the record's number, summed over the wave's lanes with the same unitig;
// kind 0 -- the wave scans the read's pairs, read by read
__global__ __launch_bounds__(256) void fin_hits_rec_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_reads, uint32_t k,
                                                           ull* counts, uint32_t n_unitigs, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap, uint32_t combine) {
    if (fin_step_withheld(ovf_count, ovf_cap, flags)) return;
    const uint32_t lane = threadIdx.x & 63u;
    const FinReadItem it = fin_read_item<false>(frec, out_offs, blockIdx.x * 256u + threadIdx.x, n_reads);
    uint32_t u = 0, cnt = 0;
    if (it.kind == 1u) {
        const uint4 a = it.a, b = it.load_b();
        uint32_t gaps = 0;
        fin_rec_gaps(a.w, a.z & 0xFFu, b.x, b.y, b.z, b.w, k, [&](uint32_t lo, uint32_t hi_excl) { gaps += hi_excl - lo; });
        u = a.x; cnt = a.w - gaps;
    }
    // ---- the records' numbers ----
    ull open = __ballot(it.kind == 1u && cnt != 0u);
    for (uint32_t round = 0; round < combine && open; round++) {
        const int lead = __ffsll((long long)open) - 1;
        const uint32_t lu = fin_bcast(u, lead);
        const bool mine = ((open >> lane) & 1ull) && u == lu;
        const uint32_t s = fin_wave_sum(mine ? cnt : 0u);   // (a record's nk is below 2^16: positions are 16 bits)
        if ((int)lane == lead) hits_add(counts, n_unitigs, flags, lu, (ull)s);
        open &= ~__ballot(mine);
    }
    if ((open >> lane) & 1ull) hits_add(counts, n_unitigs, flags, u, (ull)cnt);
    // ---- the searched reads' pairs ----
    HitsCarry c = {0xFFFFFFFFu, 0ull};
    fin_each_searched_read(it, [&](int, uint64_t lo, uint64_t hi) { hits_scan(pairs, lo, hi, counts, n_unitigs, flags, combine != 0u, c); });
    hits_flush(counts, n_unitigs, flags, c);
}

// A step that left no records: every slot of the pair array, FIN_HITS_FLAT consecutive slots per wave
__global__ __launch_bounds__(256) void fin_hits_flat_kernel(const int2* pairs, uint64_t n_pairs, ull* counts, uint32_t n_unitigs, uint32_t* flags,
                                                            const uint32_t* ovf_count, uint32_t ovf_cap, uint32_t combine) {
    if (fin_step_withheld(ovf_count, ovf_cap, flags)) return;
    const uint64_t n_spans = (n_pairs + FIN_HITS_FLAT - 1u) / FIN_HITS_FLAT;
    HitsCarry c = {0xFFFFFFFFu, 0ull};
    for (uint64_t s = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); s < n_spans; s += (uint64_t)gridDim.x * 4u) {
        const uint64_t lo = s * FIN_HITS_FLAT, hi = lo + FIN_HITS_FLAT < n_pairs ? lo + FIN_HITS_FLAT : n_pairs;
        hits_scan(pairs, lo, hi, counts, n_unitigs, flags, combine != 0u, c);
    }
    hits_flush(counts, n_unitigs, flags, c);
}

// counts: uint64[n_unitigs]; flags: one u32 (bit 0: a step without results was offered, bit 1: a unitig number outside the index).  frec null: the flat form.
// ovf_count (may be null) / ovf_cap: the step's overflow list, as batch_overrun_check reads it
extern "C" int fin_launch_hits_add(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint64_t n_pairs, uint32_t k, void* counts,
                                   uint32_t n_unitigs, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap, uint32_t combine, hipStream_t stream) {
    if (n_reads == 0 || n_unitigs == 0) return 0;
    if (frec) {
        hipLaunchKernelGGL(fin_hits_rec_kernel, dim3((n_reads + 255u) / 256u), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs, n_reads, k,
                           (ull*)counts, n_unitigs, flags, ovf_count, ovf_cap, combine);
    } else {
        if (n_pairs == 0) return 0;
        const uint64_t want = ((n_pairs + FIN_HITS_FLAT - 1u) / FIN_HITS_FLAT + 3u) / 4u;
        hipLaunchKernelGGL(fin_hits_flat_kernel, dim3((uint32_t)(want < 65536u ? want : 65536u)), dim3(256), 0, stream, (const int2*)pairs, n_pairs, (ull*)counts, n_unitigs,
                           flags, ovf_count, ovf_cap, combine);
    }
    return (int)hipGetLastError();
}
