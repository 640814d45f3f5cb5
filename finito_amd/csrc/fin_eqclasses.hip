// fin_eqclasses.hip -- EQUIVALENCE CLASSES of pseudoaligned reads (include/finito_amd.h: fin_eqclasses, fin_eqclasses_add_rows, fin_batch_add_eqclasses;
// DESIGN.md 4.15): the distinct colour rows a run produced and how many reads have each, accumulated in HBM behind fin_col_pseudo_kernel's rows.
//
// The table: open addressing, linear probing, `slots` = 2^lg entries (the power of two >= 2 max_classes):
//   tags   uint64[slots]      0 = empty, else the row's tag (its hash narrowed to tag_bits bits, never 0)
//   counts uint64[slots]      the reads of the class
//   rows   uint64[slots][W]   the class's row
//   ctr    uint64[8]          [0] rows added, [1] unaligned, [2] classes, [3] rows that went through the serial pass, [4] flags (bit 0: a row with a bit at or above
//                             n_colors -- not counted; bit 1: more than max_classes distinct rows, or a probe chain as long as the table -- the row is dropped),
//                             [5] the length of the add's collision list (0 between adds)
// and per add slot_of uint32[n_rows] and coll uint32[n_rows], scratch the accumulator keeps.
//
// NO LANE WAITS FOR ANOTHER LANE'S STORE.  A slot's tag is claimed with a 64-bit CAS; the claimant's row becomes visible later, so nothing looks at a row in the
// kernel that claims.  An add is three launches on one stream, and the kernel boundaries are the only synchronisation:
//   1  fin_ec_claim_kernel   tag = f(hash of the W words).  Probe from the tag's home slot: the CAS returns 0 -- the lane won the slot, writes its row with plain
//                            stores, bumps the class counter, slot_of[r] = s; it returns the tag -- slot_of[r] = s, a CANDIDATE; anything else -- the next slot, at
//                            most `slots` probes (then flag bit 1, the row is dropped).  All-zero rows (unaligned) and rows with stray bits are settled here.
//   2  fin_ec_count_kernel   row r is compared with rows[slot_of[r]].  Equal: counts[s] += 1, the adds of a wave combined over its DISTINCT slots (readlane of the
//                            first lane left, a ballot of the lanes with the same slot, one atomic add of the popcount -- col_add_scan's loop; a run sends millions of
//                            rows to a handful of counters).  Not equal -- two distinct rows share a tag: the row's number goes to the collision list, one
//                            wave-aggregated atomic per wave.  Rows added and unaligned: one add per wave.
//   3  fin_ec_serial_kernel  one wave in all, its loop bound the list's device-side count (0: it returns at once).  For each listed row in turn it goes on probing
//                            behind the candidate slot with full-row comparison: a matching row gets count += 1, an empty slot is claimed.  Serial, so without
//                            races and exact however many rows share a tag.  Every location it touches has ONE OWNER LANE (tags[s] and counts[s]: lane s & 63,
//                            word i of a row: lane i, the counters: lane 0), so it needs no ordering between lanes either.
// Rows are never removed, so probe chains stay valid across adds: a later add of a row that lost a tag collision finds the foreign slot first, fails the compare
// and reaches its own slot through pass 3 -- slow, and correct.  Adds do NOT commute at the memory level (a claim must not meet the half-written row of another
// add): the host runs every add behind every earlier add and reset (fin_capi.cpp).
//
// W = 1: a lane per row.  W > 1: the wave takes its 64 rows one after the other, lane i holding word i -- fin_col_pseudo_kernel's row copy: coalesced loads, a
// commutative mix per (word, index), an xor reduction over the wave, one ballot for "empty".
//
// THE WEIGHTED ADD (fin_launch_ec_add_classes): a list of {row, weight} pairs -- another accumulator's dense list -- is added as if row r had been
// added weights[r] times, and n_unaligned all-zero rows besides.  The same three passes, instantiated with WT = true (fin_ec_claimw_kernel, fin_ec_countw_kernel,
// fin_ec_serialw_kernel); the WT = false instantiations are the kernels above, unchanged:
//   1  a row of weight 0 becomes EC_DROP before anything looks at it: no class, no flag.
//   2  counts[s] += w, ONE 64-BIT ATOMIC PER ROW: a merged list is a compacted table, its rows are distinct, so combining a wave's adds over equal slots would
//      find nothing to combine (duplicate rows are legal and sum, one atomic each).  ctr[0] and ctr[1] get the wave's total weight -- fin_wave_sum64, a weight
//      may exceed 2^32 -- in one add per wave.
//   3  counts[sq] = w on a claim, += w on a match; n_done is the sum of the settled weights, ctr[3] still counts list entries.  The scalar n_unaligned is added
//      here, by lane 0 before the loop bound is looked at: an add of no rows is this launch alone.
//
// The download compacts on the device: fin_ec_occ_kernel counts the occupied slots per block of 256, fin_launch_blk_scan (fin_records.hip) makes the blocks'
// offsets and the total, fin_ec_gather_kernel writes the dense {row, reads} list.
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_wave.h"
#include "fin_rowhash.h"   // ec_mix, ec_word_hash, ec_wave_xor: the row hash, shared with fin_bootstrap.hip

#define FIN_EC_BLK 256u
#define EC_UNAL 0xFFFFFFFFu   // slot_of: the row is all zero
#define EC_DROP 0xFFFFFFFEu   // slot_of: the row is not counted (a stray bit, a full table) -- also a lane beyond n_rows

namespace {
typedef unsigned long long ull;

__device__ __forceinline__ uint64_t ec_tag(uint64_t h, uint32_t tag_bits) {
    const uint64_t t = h & ((1ull << tag_bits) - 1ull);   // tag_bits is 1 .. 63
    return t ? t : 1ull;
}
// the home slot comes from the narrowed tag: narrow tags make long chains too
__device__ __forceinline__ uint32_t ec_home(uint64_t tag, uint32_t lg) { return (uint32_t)((tag * 0x9E3779B97F4A7C15ull) >> (64u - lg)); }   // lg is 1 .. 27

// one lane claims a slot for `tag` or finds a candidate: the slot, or EC_DROP after `slots` probes; *won: the lane took an empty slot
__device__ __forceinline__ uint32_t ec_probe(ull* tags, uint32_t lg, uint64_t tag, bool* won) {
    const uint32_t slots = 1u << lg, mask = slots - 1u;
    uint32_t s = ec_home(tag, lg);
    for (uint32_t p = 0; p < slots; p++, s = (s + 1u) & mask) {
        ull t = __hip_atomic_load(tags + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t == 0ull) t = atomicCAS(tags + s, 0ull, (ull)tag);
        if (t == 0ull) { *won = true; return s; }
        if (t == tag) return s;
    }
    return EC_DROP;
}
__device__ __forceinline__ void ec_new_class(ull* ctr, uint64_t max_classes) {
    if (atomicAdd(ctr + 2, 1ull) + 1ull > max_classes) (void)atomicOr(ctr + 4, 2ull);
}

// pass 2's tail: lane's row r has slot s (or EC_UNAL / EC_DROP) and, where it has one, `eq` says that the slot's row is its own.  Wave-converged
__device__ __forceinline__ void ec_count(uint32_t r, uint32_t s, bool eq, ull* counts, ull* ctr, uint32_t* coll, uint32_t n_rows, uint32_t combine) {
    const uint32_t lane = threadIdx.x & 63u;
    const bool has = s < EC_DROP;
    const ull m_un = __ballot(s == EC_UNAL), m_eq = __ballot(has && eq), m_ne = __ballot(has && !eq);
    if (lane == 0u) {
        const ull n_un = (ull)__popcll(m_un), n_add = n_un + (ull)__popcll(m_eq);
        if (n_add) (void)atomicAdd(ctr + 0, n_add);
        if (n_un) (void)atomicAdd(ctr + 1, n_un);
    }
    if (combine) {
        ull rem = m_eq;
        while (rem) {                        // the wave's distinct slots, one atomic each
            const int src = __ffsll((long long)rem) - 1;
            const uint32_t sc = fin_bcast(s, src);
            const ull m = __ballot(has && eq && s == sc);
            rem &= ~m;
            if ((int)lane == src) (void)atomicAdd(counts + sc, (ull)__popcll(m));
        }
    } else if (has && eq) (void)atomicAdd(counts + s, 1ull);
    if (m_ne) {                              // two distinct rows under one tag: the serial pass settles them
        ull base = 0;
        if (lane == 0u) base = atomicAdd(ctr + 5, (ull)__popcll(m_ne));
        base = fin_bcast64(base, 0);
        const ull at = base + (ull)__popcll(m_ne & ((1ull << lane) - 1ull));
        if (has && !eq && at < n_rows) coll[at] = r;   // (the list starts every add empty: at < n_rows always)
    }
}
// pass 2's tail with weights: counts[s] += w where the slot's row is the lane's own, one atomic per row (the list's rows are distinct: nothing to combine); the
// wave's total weight goes to ctr[0] and ctr[1] in one add each.  w is 0 in a lane without a row and in a dropped one
__device__ __forceinline__ void ec_count_w(uint32_t r, uint32_t s, bool eq, ull w, ull* counts, ull* ctr, uint32_t* coll, uint32_t n_rows) {
    const uint32_t lane = threadIdx.x & 63u;
    const bool has = s < EC_DROP;
    const ull m_ne = __ballot(has && !eq);
    const ull n_un = fin_wave_sum64(s == EC_UNAL ? w : 0ull), n_add = n_un + fin_wave_sum64(has && eq ? w : 0ull);
    if (lane == 0u) {
        if (n_add) (void)atomicAdd(ctr + 0, n_add);
        if (n_un) (void)atomicAdd(ctr + 1, n_un);
    }
    if (has && eq) (void)atomicAdd(counts + s, w);
    if (m_ne) {                              // two distinct rows under one tag: the serial pass settles them
        ull base = 0;
        if (lane == 0u) base = atomicAdd(ctr + 5, (ull)__popcll(m_ne));
        base = fin_bcast64(base, 0);
        const ull at = base + (ull)__popcll(m_ne & ((1ull << lane) - 1ull));
        if (has && !eq && at < n_rows) coll[at] = r;   // (the list starts every add empty: at < n_rows always)
    }
}
}  // namespace

// pass 1.  rows: uint64[n_rows * W]; stray: the bits of word W - 1 that no colour has (0: none).  WT: weights[n_rows], a row of weight 0 is dropped unseen
template <bool WT>
__device__ __forceinline__ void ec_claim(const ull* rows, const ull* weights, uint32_t n_rows, uint32_t W, ull stray, ull* tags, ull* tab_rows, uint32_t lg,
                                         uint64_t max_classes, uint32_t tag_bits, ull* ctr, uint32_t* slot_of) {
    const uint32_t r = blockIdx.x * FIN_EC_BLK + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t r0 = r - lane;           // the wave's first row
    uint32_t mine = EC_DROP;
    const bool idle = WT && r < n_rows && weights[r] == 0ull;   // (WT false: a constant)
    if (W == 1u) {
        if (r < n_rows && !idle) {
            const ull word = rows[r];
            if (word == 0ull) mine = EC_UNAL;
            else if (word & stray) (void)atomicOr(ctr + 4, 1ull);
            else {
                bool won = false;
                mine = ec_probe(tags, lg, ec_tag(ec_word_hash(word, 0u), tag_bits), &won);
                if (won) { tab_rows[mine] = word; ec_new_class(ctr, max_classes); }
                if (mine == EC_DROP) (void)atomicOr(ctr + 4, 2ull);
            }
        }
    } else {
        const uint32_t n_here = r0 < n_rows ? min(64u, n_rows - r0) : 0u;   // wave-uniform
        const ull m_idle = WT ? __ballot(idle) : 0ull;
        ull next = 0ull;                    // the row to come, loaded a row ahead
        if (n_here != 0u && lane < W) next = rows[(uint64_t)r0 * W + lane];
        for (uint32_t i = 0; i < n_here; i++) {
            const ull word = next;
            next = 0ull;
            if (i + 1u < n_here && lane < W) next = rows[(uint64_t)(r0 + i + 1u) * W + lane];
            uint32_t res = EC_DROP;
            if (WT && ((m_idle >> i) & 1ull)) {}
            else if (__ballot(word != 0ull) == 0ull) res = EC_UNAL;
            else if (__ballot(lane == W - 1u && (word & stray) != 0ull)) { if (lane == 0u) (void)atomicOr(ctr + 4, 1ull); }
            else {
                const uint64_t tag = ec_tag(ec_wave_xor(lane < W ? ec_word_hash(word, lane) : 0ull), tag_bits);
                bool won = false;
                if (lane == 0u) res = ec_probe(tags, lg, tag, &won);
                res = fin_bcast(res, 0);
                if (fin_bcast((uint32_t)won, 0)) {
                    if (lane < W) tab_rows[(uint64_t)res * W + lane] = word;
                    if (lane == 0u) ec_new_class(ctr, max_classes);
                }
                if (res == EC_DROP && lane == 0u) (void)atomicOr(ctr + 4, 2ull);
            }
            if (lane == i) mine = res;
        }
    }
    if (r < n_rows) slot_of[r] = mine;
}
__global__ __launch_bounds__(256) void fin_ec_claim_kernel(const ull* rows, uint32_t n_rows, uint32_t W, ull stray, ull* tags, ull* tab_rows, uint32_t lg,
                                                           uint64_t max_classes, uint32_t tag_bits, ull* ctr, uint32_t* slot_of) {
    ec_claim<false>(rows, nullptr, n_rows, W, stray, tags, tab_rows, lg, max_classes, tag_bits, ctr, slot_of);
}
__global__ __launch_bounds__(256) void fin_ec_claimw_kernel(const ull* rows, const ull* weights, uint32_t n_rows, uint32_t W, ull stray, ull* tags, ull* tab_rows,
                                                            uint32_t lg, uint64_t max_classes, uint32_t tag_bits, ull* ctr, uint32_t* slot_of) {
    ec_claim<true>(rows, weights, n_rows, W, stray, tags, tab_rows, lg, max_classes, tag_bits, ctr, slot_of);
}

// pass 2: is the row of the lane's slot s (or EC_UNAL / EC_DROP: no) its own row r?  Wave-converged
__device__ __forceinline__ bool ec_same(const ull* rows, uint32_t r, uint32_t s, uint32_t W, const ull* tab_rows) {
    const uint32_t lane = threadIdx.x & 63u, r0 = r - lane;
    bool eq = false;
    if (W == 1u) {
        if (s < EC_DROP) eq = rows[r] == tab_rows[s];
    } else {
        ull todo = __ballot(s < EC_DROP);
        ull a = 0ull, b = 0ull;             // the pair to come, loaded a row ahead
        if (todo) {
            const int src = __ffsll((long long)todo) - 1;
            const uint32_t ss = fin_bcast(s, src);
            if (lane < W) { a = rows[(uint64_t)(r0 + (uint32_t)src) * W + lane]; b = tab_rows[(uint64_t)ss * W + lane]; }
        }
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const ull x = a, y = b;
            a = b = 0ull;
            if (todo) {
                const int nx = __ffsll((long long)todo) - 1;
                const uint32_t ss = fin_bcast(s, nx);
                if (lane < W) { a = rows[(uint64_t)(r0 + (uint32_t)nx) * W + lane]; b = tab_rows[(uint64_t)ss * W + lane]; }
            }
            const bool same = __ballot(x != y) == 0ull;
            if ((int)lane == src) eq = same;
        }
    }
    return eq;
}
__global__ __launch_bounds__(256) void fin_ec_count_kernel(const ull* rows, uint32_t n_rows, uint32_t W, const ull* tab_rows, ull* counts, ull* ctr,
                                                           const uint32_t* slot_of, uint32_t* coll, uint32_t combine) {
    const uint32_t r = blockIdx.x * FIN_EC_BLK + threadIdx.x;
    const uint32_t s = r < n_rows ? slot_of[r] : EC_DROP;
    ec_count(r, s, ec_same(rows, r, s, W, tab_rows), counts, ctr, coll, n_rows, combine);
}
__global__ __launch_bounds__(256) void fin_ec_countw_kernel(const ull* rows, const ull* weights, uint32_t n_rows, uint32_t W, const ull* tab_rows, ull* counts, ull* ctr,
                                                            const uint32_t* slot_of, uint32_t* coll) {
    const uint32_t r = blockIdx.x * FIN_EC_BLK + threadIdx.x;
    const uint32_t s = r < n_rows ? slot_of[r] : EC_DROP;
    const ull w = s != EC_DROP ? weights[r] : 0ull;   // (s is EC_DROP in a lane beyond n_rows)
    ec_count_w(r, s, ec_same(rows, r, s, W, tab_rows), w, counts, ctr, coll, n_rows);
}

// pass 3: one wave.  Lane s & 63 owns tags[s] and counts[s], lane i word i of every row, lane 0 the counters.  WT: a listed row settles with its weight, and
// n_unaligned all-zero rows are counted besides
template <bool WT>
__device__ __forceinline__ void ec_serial(const ull* rows, const ull* weights, uint32_t n_rows, ull n_unaligned, uint32_t W, ull* tags, ull* counts, ull* tab_rows, uint32_t lg,
                                          uint64_t max_classes, ull* ctr, const uint32_t* slot_of, const uint32_t* coll) {
    const uint32_t lane = threadIdx.x;
    if (WT && lane == 0u && n_unaligned) { ctr[0] += n_unaligned; ctr[1] += n_unaligned; }   // (lane 0 owns the counters; its later ctr[0] += is behind this in program order)
    const uint64_t n = min((uint64_t)ctr[5], (uint64_t)n_rows);
    if (n == 0ull) return;
    const uint32_t slots = 1u << lg, mask = slots - 1u, width = min(64u, slots);
    uint64_t n_done = 0, n_new = 0;         // (kept in every lane, used by lane 0)
    bool full = false;
    for (uint64_t j = 0; j < n; j++) {
        const uint32_t r = coll[j], cand = slot_of[r];
        const ull word = lane < W ? rows[(uint64_t)r * W + lane] : 0ull;
        const ull w = WT ? weights[r] : 1ull;
        const ull tag = fin_bcast64(lane == (cand & 63u) ? tags[cand] : 0ull, (int)(cand & 63u));   // the candidate's tag is the row's
        uint32_t s = (cand + 1u) & mask;
        bool done = false;
        for (uint64_t probed = 0; probed < slots && !done;) {
            const uint32_t b = s & ~(width - 1u);   // the window of `width` slots around s: lane q looks at slot b + q
            const bool in = lane < width && b + lane >= s;
            const ull t = in ? tags[b + lane] : ~0ull;
            ull cm = __ballot(in && (t == 0ull || t == tag));
            while (cm && !done) {
                const int q = __ffsll((long long)cm) - 1;
                cm &= cm - 1ull;
                const uint32_t sq = b + (uint32_t)q;
                if (fin_bcast64(t, q) == 0ull) {      // an empty slot ends the chain: the row is new
                    if ((int)lane == q) { tags[sq] = tag; counts[sq] = w; }
                    if (lane < W) tab_rows[(uint64_t)sq * W + lane] = word;
                    n_new++; n_done += w; done = true;
                } else if (__ballot(lane < W && tab_rows[(uint64_t)sq * W + lane] != word) == 0ull) {
                    if ((int)lane == q) counts[sq] += w;
                    n_done += w; done = true;
                }
            }
            probed += (uint64_t)(b + width - s);
            s = (b + width) & mask;
        }
        if (!done) full = true;
    }
    if (lane == 0u) {
        const ull classes = ctr[2] + n_new;
        ctr[0] += n_done; ctr[2] = classes; ctr[3] += n;
        if (full || classes > max_classes) ctr[4] |= 2ull;
        ctr[5] = 0ull;
    }
}
__global__ __launch_bounds__(64) void fin_ec_serial_kernel(const ull* rows, uint32_t n_rows, uint32_t W, ull* tags, ull* counts, ull* tab_rows, uint32_t lg, uint64_t max_classes,
                                                           ull* ctr, const uint32_t* slot_of, const uint32_t* coll) {
    ec_serial<false>(rows, nullptr, n_rows, 0ull, W, tags, counts, tab_rows, lg, max_classes, ctr, slot_of, coll);
}
__global__ __launch_bounds__(64) void fin_ec_serialw_kernel(const ull* rows, const ull* weights, uint32_t n_rows, ull n_unaligned, uint32_t W, ull* tags, ull* counts,
                                                            ull* tab_rows, uint32_t lg, uint64_t max_classes, ull* ctr, const uint32_t* slot_of, const uint32_t* coll) {
    ec_serial<true>(rows, weights, n_rows, n_unaligned, W, tags, counts, tab_rows, lg, max_classes, ctr, slot_of, coll);
}

// blk_sum[block] = the occupied slots among the block's 256
__global__ __launch_bounds__(256) void fin_ec_occ_kernel(const ull* tags, uint32_t slots, uint32_t* blk_sum) {
    __shared__ uint32_t lds_w[4];
    const uint32_t s = blockIdx.x * FIN_EC_BLK + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const ull m = __ballot(s < slots && tags[s] != 0ull);
    if (lane == 0u) lds_w[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) blk_sum[blockIdx.x] = lds_w[0] + lds_w[1] + lds_w[2] + lds_w[3];
}

// out_rows[d][0 .. W), out_reads[d] = the d-th occupied slot's row and count, d in slot order
__global__ __launch_bounds__(256) void fin_ec_gather_kernel(const ull* tags, const ull* counts, const ull* tab_rows, uint32_t slots, uint32_t W, const uint64_t* blk_off,
                                                            ull* out_rows, ull* out_reads) {
    __shared__ uint32_t lds_w[4];
    const uint32_t s = blockIdx.x * FIN_EC_BLK + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool occ = s < slots && tags[s] != 0ull;
    const ull m = __ballot(occ);
    if (lane == 0u) lds_w[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!occ) return;
    uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t q = 0; q < wave; q++) before += lds_w[q];
    const uint64_t d = blk_off[blockIdx.x] + before;
    for (uint32_t w = 0; w < W; w++) out_rows[d * W + w] = tab_rows[(uint64_t)s * W + w];
    out_reads[d] = counts[s];
}

// rows: uint64[n_rows * W], n_rows < 2^31; tags / counts / tab_rows / ctr: the table (2^lg slots, 1 <= lg <= 27); slot_of, coll: n_rows u32 each.  Three launches
extern "C" int fin_launch_ec_add(const void* rows, uint32_t n_rows, uint32_t W, uint32_t n_colors, void* tags, void* counts, void* tab_rows, uint32_t lg,
                                 uint64_t max_classes, uint32_t tag_bits, uint32_t combine, void* ctr, uint32_t* slot_of, uint32_t* coll, hipStream_t stream) {
    const uint32_t nb = (n_rows + FIN_EC_BLK - 1u) / FIN_EC_BLK;
    if (nb == 0) return 0;
    if (W == 0 || W > 64u || lg == 0 || lg > 27u || tag_bits == 0 || tag_bits > 63u) return (int)hipErrorInvalidValue;
    const ull stray = (n_colors & 63u) ? ~0ull << (n_colors & 63u) : 0ull;
    hipLaunchKernelGGL(fin_ec_claim_kernel, dim3(nb), dim3(256), 0, stream, (const ull*)rows, n_rows, W, stray, (ull*)tags, (ull*)tab_rows, lg, max_classes, tag_bits,
                       (ull*)ctr, slot_of);
    hipLaunchKernelGGL(fin_ec_count_kernel, dim3(nb), dim3(256), 0, stream, (const ull*)rows, n_rows, W, (const ull*)tab_rows, (ull*)counts, (ull*)ctr,
                       (const uint32_t*)slot_of, coll, combine);
    hipLaunchKernelGGL(fin_ec_serial_kernel, dim3(1), dim3(64), 0, stream, (const ull*)rows, n_rows, W, (ull*)tags, (ull*)counts, (ull*)tab_rows, lg, max_classes, (ull*)ctr,
                       (const uint32_t*)slot_of, (const uint32_t*)coll);
    return (int)hipGetLastError();
}
// the weighted add: row r counts weights[r] times (uint64[n_rows], 0: the row is skipped), and n_unaligned all-zero rows besides.  The same table arguments and
// scratch; the count pass has no combine.  Three launches; the serial pass alone where there are no rows
extern "C" int fin_launch_ec_add_classes(const void* rows, const void* weights, uint32_t n_rows, uint64_t n_unaligned, uint32_t W, uint32_t n_colors, void* tags, void* counts,
                                         void* tab_rows, uint32_t lg, uint64_t max_classes, uint32_t tag_bits, void* ctr, uint32_t* slot_of, uint32_t* coll,
                                         hipStream_t stream) {
    const uint32_t nb = (n_rows + FIN_EC_BLK - 1u) / FIN_EC_BLK;
    if (nb == 0 && n_unaligned == 0) return 0;
    if (W == 0 || W > 64u || lg == 0 || lg > 27u || tag_bits == 0 || tag_bits > 63u) return (int)hipErrorInvalidValue;
    const ull stray = (n_colors & 63u) ? ~0ull << (n_colors & 63u) : 0ull;
    if (nb != 0) {
        hipLaunchKernelGGL(fin_ec_claimw_kernel, dim3(nb), dim3(256), 0, stream, (const ull*)rows, (const ull*)weights, n_rows, W, stray, (ull*)tags, (ull*)tab_rows, lg,
                           max_classes, tag_bits, (ull*)ctr, slot_of);
        hipLaunchKernelGGL(fin_ec_countw_kernel, dim3(nb), dim3(256), 0, stream, (const ull*)rows, (const ull*)weights, n_rows, W, (const ull*)tab_rows, (ull*)counts,
                           (ull*)ctr, (const uint32_t*)slot_of, coll);
    }
    hipLaunchKernelGGL(fin_ec_serialw_kernel, dim3(1), dim3(64), 0, stream, (const ull*)rows, (const ull*)weights, n_rows, (ull)n_unaligned, W, (ull*)tags, (ull*)counts,
                       (ull*)tab_rows, lg, max_classes, (ull*)ctr, (const uint32_t*)slot_of, (const uint32_t*)coll);
    return (int)hipGetLastError();
}
extern "C" uint32_t fin_ec_blocks(uint32_t slots) { return (slots + FIN_EC_BLK - 1u) / FIN_EC_BLK; }
// blk_sum: fin_ec_blocks() u32; blk_off: as many u64; *total = the occupied slots
extern "C" int fin_launch_ec_occupied(const void* tags, uint32_t slots, uint32_t* blk_sum, uint64_t* blk_off, uint64_t* total, hipStream_t stream) {
    const uint32_t nb = fin_ec_blocks(slots);
    hipLaunchKernelGGL(fin_ec_occ_kernel, dim3(nb), dim3(256), 0, stream, (const ull*)tags, slots, blk_sum);
    return fin_launch_blk_scan(blk_sum, nb, blk_off, total, stream);
}
// out_rows: room for *total rows of W words; out_reads: as many u64
extern "C" int fin_launch_ec_gather(const void* tags, const void* counts, const void* tab_rows, uint32_t slots, uint32_t W, const uint64_t* blk_off, void* out_rows,
                                    void* out_reads, hipStream_t stream) {
    hipLaunchKernelGGL(fin_ec_gather_kernel, dim3(fin_ec_blocks(slots)), dim3(256), 0, stream, (const ull*)tags, (const ull*)counts, (const ull*)tab_rows, slots, W,
                       blk_off, (ull*)out_rows, (ull*)out_reads);
    return (int)hipGetLastError();
}
