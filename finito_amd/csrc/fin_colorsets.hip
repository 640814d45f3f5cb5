// fin_colorsets.hip -- DEDUPLICATED COLOUR SETS: the compact state of fin_colors (include/finito_amd.h: fin_colors_compact, fin_colors_expand).
// The unitigs of a graph over many references carry few distinct colour rows; the compact state stores each distinct row once:
//   set_of[n_unitigs] u32 and sets[n_sets + 1][W] u64; sets[0] is the empty row, set_of[u] == 0 iff unitig u's row is empty, rows 1 .. n_sets are non-empty and
//   pairwise distinct, sets[set_of[u]] is unitig u's row bit for bit.  The order of the ids 1 .. n_sets is unspecified.
//
// The matrix is immutable while this runs (the caller ordered every add, upload and reset before it), so a table slot need not hold a row: one 64-bit word
// {tag << 32 | representative unitig + 1}, 0 = free, claimed by ONE compare-and-swap.  tag = bits 33 .. 63 of the row's hash (fin_rowhash.h) narrowed to tag_bits
// bits (option "colorsets_tag_bits": tests force distinct rows under one tag); the home slot is a function of the TAG, ~(ec_mix(tag) >> 7) & (slots - 1), so rows of
// one tag walk one chain -- and tag 0, whose home is the LAST slot (ec_mix(0) = 0), wraps with its second row: narrow tags always exercise the wrap.  Open addressing, linear probing with wrap, over slots = 2^lg >= 2 max_sets.
//   1 fin_cs_claim_kernel   a lane per unitig.  The hash: W = 1 a lane hashes its own word; W > 1 the wave takes its 64 unitigs in turn, lane i word i (coalesced),
//                           an xor across the wave.  An empty row gets no slot.  Then every lane probes: a free slot -- CAS; won: the lane's unitig is the set's
//                           representative.  A slot with the lane's tag (found by the load or returned by the lost CAS): the lane compares its row with
//                           bits[representative] AT ONCE -- that row was in memory before the launch, nothing is waited for; equal: this is the lane's slot;
//                           not equal (a foreign row under the tag): probe on.  After `slots` probes, or once more than max_sets slots are claimed: flag.
//   2 fin_cs_occ_kernel     occupied slots per block of 256, then fin_launch_blk_scan (fin_records.hip): the blocks' offsets and the total = n_sets
//   3 fin_cs_gather_kernel  id = 1 + the rank of the occupied slot -> slot_id[slot]; sets[id] = bits[representative], the wave moves a row lane i word i; row 0 zeroed
//   4 fin_cs_setof_kernel   set_of[u] = slot_id[slot_of[u]], 0 for an empty row
// No lane waits for another's store, no serial pass: a tag collision costs one row compare.  fin_cs_expand_kernel is the way back: bits[u] = sets[set_of[u]].
// ctr: 4 u64 -- [0] slots claimed, [1] rows that met a foreign row under their tag, [2] the longest probe (slots looked at behind the home slot), [3] flags
// (bit 0: the table or max_sets overran).
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_rowhash.h"
#include "fin_wave.h"

#define FIN_CS_BLK 256u
#define FIN_CS_NONE 0xFFFFFFFFu   // slot_of of an empty row

namespace {
typedef unsigned long long ull;

__device__ __forceinline__ bool cs_row_equal(const ull* bits, uint32_t W, uint32_t a, uint32_t b) {
    if (a == b) return true;
    const ull* ra = bits + (uint64_t)a * W;
    const ull* rb = bits + (uint64_t)b * W;
    for (uint32_t w = 0; w < W; w++) if (ra[w] != rb[w]) return false;
    return true;
}
}  // namespace

__global__ __launch_bounds__(256) void fin_cs_claim_kernel(const ull* bits, uint32_t n_unitigs, uint32_t W, ull* slots, uint32_t lg, uint32_t tag_bits, uint64_t max_sets,
                                                           uint32_t* slot_of, ull* ctr) {
    const uint32_t u = blockIdx.x * FIN_CS_BLK + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t u0 = u - lane;           // the wave's first unitig
    uint64_t h = 0;
    bool ne = false;
    if (W == 1u) {
        if (u < n_unitigs) { const ull w = bits[u]; ne = w != 0ull; h = ec_word_hash(w, 0u); }
    } else {
        const uint32_t n_here = u0 < n_unitigs ? min(64u, n_unitigs - u0) : 0u;
        for (uint32_t i = 0; i < n_here; i++) {
            const ull w = lane < W ? bits[(uint64_t)(u0 + i) * W + lane] : 0ull;
            const uint64_t hi = ec_wave_xor(lane < W ? ec_word_hash(w, lane) : 0ull);
            const bool nei = __ballot(w != 0ull) != 0ull;
            if (lane == i) { h = hi; ne = nei; }
        }
    }
    const uint32_t mask = (1u << lg) - 1u;
    const uint32_t tag = (uint32_t)(h >> 33) & (uint32_t)((1ull << tag_bits) - 1ull);
    const ull mine = ((ull)tag << 32) | (ull)(u + 1u);
    uint32_t s = ~(uint32_t)(ec_mix((uint64_t)tag) >> 7) & mask, probes = 0, found = FIN_CS_NONE;
    bool foreign = false, over = false;
    if (u < n_unitigs && ne) {
        for (;;) {
            ull cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == 0ull) {
                ull expected = 0ull;
                if (__hip_atomic_compare_exchange_strong(slots + s, &expected, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    found = s;
                    if (__hip_atomic_fetch_add(ctr + 0, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= max_sets) over = true;
                    break;
                }
                cur = expected;             // another lane's claim
            }
            if ((uint32_t)(cur >> 32) == tag) {
                if (cs_row_equal(bits, W, u, (uint32_t)cur - 1u)) { found = s; break; }
                foreign = true;
            }
            if (++probes > mask) { over = true; break; }   // every slot was looked at
            s = (s + 1u) & mask;
        }
    }
    if (u < n_unitigs) slot_of[u] = found;
    // the counters: one atomic each per wave
    const uint32_t n_foreign = (uint32_t)__popcll(__ballot(foreign));
    const uint32_t longest = fin_wave_max(probes);
    const bool any_over = __ballot(over) != 0ull;
    if (lane == 0u) {
        if (n_foreign) (void)__hip_atomic_fetch_add(ctr + 1, (ull)n_foreign, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (longest) (void)__hip_atomic_fetch_max(ctr + 2, (ull)longest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (any_over) (void)__hip_atomic_fetch_or(ctr + 3, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void fin_cs_occ_kernel(const ull* slots, uint32_t n_slots, uint32_t* blk_sum) {
    __shared__ uint32_t lds_w[4];
    const uint32_t s = blockIdx.x * FIN_CS_BLK + threadIdx.x;
    const uint32_t t = fin_block_sum4(s < n_slots && slots[s] != 0ull ? 1u : 0u, lds_w);
    if (threadIdx.x == 0u) blk_sum[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void fin_cs_gather_kernel(const ull* bits, uint32_t W, const ull* slots, uint32_t n_slots, const uint64_t* blk_off, uint32_t* slot_id,
                                                            ull* sets) {
    __shared__ uint32_t lds_w[4];
    const uint32_t s = blockIdx.x * FIN_CS_BLK + threadIdx.x, lane = threadIdx.x & 63u;
    const ull cur = s < n_slots ? slots[s] : 0ull;
    const bool occ = cur != 0ull;
    const uint32_t id = 1u + (uint32_t)blk_off[blockIdx.x] + fin_block_exclusive4(occ ? 1u : 0u, lds_w, nullptr);
    const uint32_t rep = (uint32_t)cur - 1u;
    if (occ) slot_id[s] = id;
    if (s < W) sets[s] = 0ull;              // row 0: the empty set
    if (W == 1u) {
        if (occ) sets[id] = bits[rep];
    } else {
        fin_each_lane(occ, [&](int src) {
            const uint32_t ids = fin_bcast(id, src), reps = fin_bcast(rep, src);
            if (lane < W) sets[(uint64_t)ids * W + lane] = bits[(uint64_t)reps * W + lane];
        });
    }
}

__global__ __launch_bounds__(256) void fin_cs_setof_kernel(const uint32_t* slot_of, const uint32_t* slot_id, uint32_t n_unitigs, uint32_t* set_of) {
    const uint32_t u = blockIdx.x * FIN_CS_BLK + threadIdx.x;
    if (u >= n_unitigs) return;
    const uint32_t s = slot_of[u];
    set_of[u] = s == FIN_CS_NONE ? 0u : slot_id[s];
}

// bits[u][w] = sets[set_of[u]][w]: a thread per word, the stores coalesced
__global__ __launch_bounds__(256) void fin_cs_expand_kernel(const uint32_t* set_of, const ull* sets, uint64_t n_words, uint32_t W, ull* bits) {
    const uint64_t i = (uint64_t)blockIdx.x * FIN_CS_BLK + threadIdx.x;
    if (i >= n_words) return;
    const uint64_t u = i / W;
    bits[i] = sets[(uint64_t)set_of[u] * W + (i - u * W)];
}

extern "C" uint32_t fin_cs_blocks(uint32_t slots) { return (slots + FIN_CS_BLK - 1u) / FIN_CS_BLK; }
// slots: 2^lg u64 and ctr: 4 u64, both zeroed by the caller; slot_of: n_unitigs u32; blk_sum: fin_cs_blocks(2^lg) u32, blk_off as many u64; *total = the
// occupied slots = n_sets.  The caller reads ctr and *total back before it goes on
extern "C" int fin_launch_cs_claim(const void* bits, uint32_t n_unitigs, uint32_t W, void* slots, uint32_t lg, uint32_t tag_bits, uint64_t max_sets, uint32_t* slot_of,
                                   void* ctr, uint32_t* blk_sum, uint64_t* blk_off, uint64_t* total, hipStream_t stream) {
    if (W == 0 || W > 64u || lg == 0 || lg > 27u || tag_bits == 0 || tag_bits > 31u || n_unitigs >= 0x80000000u) return (int)hipErrorInvalidValue;
    const uint32_t nb = fin_cs_blocks(n_unitigs), n_slots = 1u << lg, nsb = fin_cs_blocks(n_slots);
    if (nb) hipLaunchKernelGGL(fin_cs_claim_kernel, dim3(nb), dim3(256), 0, stream, (const ull*)bits, n_unitigs, W, (ull*)slots, lg, tag_bits, max_sets, slot_of, (ull*)ctr);
    hipLaunchKernelGGL(fin_cs_occ_kernel, dim3(nsb), dim3(256), 0, stream, (const ull*)slots, n_slots, blk_sum);
    const int rc = (int)hipGetLastError();
    return rc ? rc : fin_launch_blk_scan(blk_sum, nsb, blk_off, total, stream);
}
// slot_id: 2^lg u32 of scratch; sets: room for (*total + 1) rows of W words; set_of: n_unitigs u32
extern "C" int fin_launch_cs_gather(const void* bits, uint32_t n_unitigs, uint32_t W, const void* slots, uint32_t lg, const uint32_t* slot_of, const uint64_t* blk_off,
                                    uint32_t* slot_id, void* sets, uint32_t* set_of, hipStream_t stream) {
    const uint32_t nb = fin_cs_blocks(n_unitigs), n_slots = 1u << lg;
    hipLaunchKernelGGL(fin_cs_gather_kernel, dim3(fin_cs_blocks(n_slots)), dim3(256), 0, stream, (const ull*)bits, W, (const ull*)slots, n_slots, blk_off, slot_id,
                       (ull*)sets);
    if (nb) hipLaunchKernelGGL(fin_cs_setof_kernel, dim3(nb), dim3(256), 0, stream, slot_of, slot_id, n_unitigs, set_of);
    return (int)hipGetLastError();
}
// bits: uint64[n_unitigs * W]
extern "C" int fin_launch_cs_expand(const uint32_t* set_of, const void* sets, uint32_t n_unitigs, uint32_t W, void* bits, hipStream_t stream) {
    const uint64_t n_words = (uint64_t)n_unitigs * W;
    const uint64_t nb = (n_words + FIN_CS_BLK - 1u) / FIN_CS_BLK;   // (< 2^31 * 64 / 256 = 2^29 blocks)
    if (nb == 0) return 0;
    hipLaunchKernelGGL(fin_cs_expand_kernel, dim3((uint32_t)nb), dim3(256), 0, stream, set_of, (const ull*)sets, n_words, W, (ull*)bits);
    return (int)hipGetLastError();
}
