// fin_links.hip -- the LINKS of a run: which junctions of the unitig graph the reads crossed, and how often (include/finito_amd.h: LINKS -- the definition is
// stated there and nowhere else).  Every sibling looks inside one unitig at a time; this file counts the steps between them: two neighbouring
// found slots of a read that do not continue each other, keyed by the unordered pair of their places.
//
// What is read (the frame is fin_wave.h's): a lane per read.  A kind-1 record is one diagonal of one unitig -- its found slots step by one, its gaps are absent
// slots -- and a kind-2 read has no found slot: neither can hold a transition, both return behind the one 16-byte load of fin_read_item<false>, and b is never
// loaded.  A kind-0 read's pairs are scanned by the wave, a row of 64 slots at a time: the slot before comes by __shfl_up, the last slot of the row before is
// carried wave-uniform (FinSegCarry), and a read begins with an empty carry, so the last slot of one read never meets the first slot of the next.  Where the step
// left no records every read is a kind-0 read and is scanned the same way, through out_offs: there is no flat form, which would link across reads.
//
// The table: cap slots of {key, count}, cap a power of two.  A lane with a transition loads its two ends_p entries, checks both places and inserts itself: from
// the key's home slot it tries a 64-bit CAS of the key against the empty key; the slot holds its key -- claimed now, or found there -- and it adds 1 to the
// count; the slot holds another key and it goes on to the next.  At most cap probes, then flag bit 2.  A claim counts in n_distinct; one that brings it above
// max_links sets flag bit 2 (the entry stays: the download refuses anyway).  CAS and adds are relaxed, agent scope.  No thread waits for another: a claimed
// slot's count may be 0 for a moment, and nobody reads counts before the kernel has ended.  Integer adds commute: the table's CONTENT is exact whatever order the
// lanes arrive in; which slot a key lands in is not, and the download sorts.  Equal keys of a row are not combined before the atomics (not measured to pay).
//
// The download compacts on the device: fin_links_count_kernel counts per block of 256 slots those to keep, fin_launch_blk_scan (fin_records.hip) makes the blocks'
// offsets, fin_links_write_kernel turns each kept key back into {u_a, off_a, u_b, off_b, count} -- the unitig of a place by binary search in ends_p, as
// fin_depth_stat_kernel finds one.  No block waits for another.
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_linkhash.h"
#include "fin_wave.h"

#define FIN_LINKS_BLK 256u

namespace {
typedef unsigned long long ull;

struct LinkOut { uint32_t u_a, off_a, u_b, off_b; ull count; };   // fin_link
static_assert(sizeof(LinkOut) == 24, "fin_link is 24 bytes");

__device__ __forceinline__ ull* links_ctr(ull* tab, uint32_t cap) { return tab + 2ull * cap; }
__device__ __forceinline__ uint32_t* links_flags(ull* tab, uint32_t cap) { return (uint32_t*)(tab + 2ull * cap + 1u); }
__device__ __forceinline__ void links_flag(uint32_t* flags, uint32_t bit) { (void)__hip_atomic_fetch_or(flags, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a lane: one transition with this key.  Every slot index is masked by cap - 1
__device__ __forceinline__ void links_insert(ull* tab, uint32_t cap, ull max_links, ull key) {
    const uint32_t mask = cap - 1u;
    uint32_t s = (uint32_t)fin_link_mix(key) & mask;
    for (uint32_t probe = 0; probe < cap; probe++, s = (s + 1u) & mask) {
        ull* const slot = tab + 2ull * s;
        ull seen = FIN_LINK_EMPTY;
        if (__hip_atomic_compare_exchange_strong(slot, &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            seen = key;
            if (__hip_atomic_fetch_add(links_ctr(tab, cap), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1ull > max_links) links_flag(links_flags(tab, cap), 4u);
        }
        if (seen == key) {
            (void)__hip_atomic_fetch_add(slot + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
    links_flag(links_flags(tab, cap), 4u);
}

// the unitig whose text holds place g < total_len: the last u in [0, n_unitigs) with ends_p[u] <= g (ends_p[0] = 0)
__device__ __forceinline__ uint32_t links_unitig_of(const uint32_t* ends_p, uint32_t n_unitigs, uint32_t g) {
    uint32_t lo = 0, hi = n_unitigs;
    while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (ends_p[mid] <= g) lo = mid; else hi = mid; }
    return lo;
}
// a slot of the table as the download sees it: kept iff occupied and count >= min_count
__device__ __forceinline__ bool links_slot(const ull* tab, uint32_t cap, uint32_t s, ull min_count, ull& key, ull& count) {
    key = FIN_LINK_EMPTY; count = 0;
    if (s < cap) { const ulonglong2 e = ((const ulonglong2*)tab)[s]; key = e.x; count = e.y; }
    return key != FIN_LINK_EMPTY && count >= min_count;
}
}  // namespace

__global__ __launch_bounds__(256) void fin_links_clear_kernel(ull* tab, uint32_t cap) {
    const uint32_t s = blockIdx.x * FIN_LINKS_BLK + threadIdx.x;
    if (s < cap) ((ulonglong2*)tab)[s] = make_ulonglong2(FIN_LINK_EMPTY, 0ull);
    if (s == 0u) ((ulonglong2*)tab)[cap] = make_ulonglong2(0ull, 0ull);   // n_distinct, flags
}

// A lane per read; the wave scans its lanes' searched reads one after the other
__global__ __launch_bounds__(256) void fin_links_add_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_reads, const uint32_t* ends_p,
                                                            uint32_t n_unitigs, uint64_t total_len, ull* tab, uint32_t cap, ull max_links, const uint32_t* ovf_count,
                                                            uint32_t ovf_cap) {
    if (fin_step_withheld(ovf_count, ovf_cap, links_flags(tab, cap))) return;
    const FinReadItem it = fin_read_item<false>(frec, out_offs, blockIdx.x * 256u + threadIdx.x, n_reads);
    const uint32_t lane = threadIdx.x & 63u;
    fin_each_searched_read(it, [&](int, uint64_t lo, uint64_t hi) {
        FinSegCarry c;   // a read begins with no slot before it
        fin_each_pair_row(pairs, lo, hi, [&](uint64_t, uint64_t, int2 p) {
            const uint32_t u = (uint32_t)p.x, off = (uint32_t)p.y;   // (-1,-1) in a lane beyond hi: absent
            const bool found = u != 0xFFFFFFFFu;
            uint32_t up = (uint32_t)__shfl_up((int)u, 1), offp = (uint32_t)__shfl_up((int)off, 1);
            if (lane == 0u) { up = c.pu; offp = c.poff; }
            int link;
            (void)fin_seg_head(u, off, found, c, link);
            if (found && up != 0xFFFFFFFFu && link == 0) {
                // both ends' places, checked before anything is inserted
                bool ok = u < n_unitigs && up < n_unitigs;
                uint64_t ga = 0, gb = 0;
                if (ok) { ga = (uint64_t)ends_p[up] + offp; gb = (uint64_t)ends_p[u] + off; ok = ga < total_len && gb < total_len; }
                if (ok) links_insert(tab, cap, max_links, fin_link_key((uint32_t)ga, (uint32_t)gb));
                else links_flag(links_flags(tab, cap), 2u);
            }
            fin_seg_next_row(c, u, off, link);
        });
    });
}

// blk_sum[block] = the block's slots to keep; stats += {the sum of every occupied slot's count, the occupied slots whose two places are equal}
__global__ __launch_bounds__(256) void fin_links_count_kernel(const ull* tab, uint32_t cap, ull min_count, uint32_t* blk_sum, ull* stats) {
    __shared__ uint32_t lds_w[4];
    ull key, count;
    const bool keep = links_slot(tab, cap, blockIdx.x * FIN_LINKS_BLK + threadIdx.x, min_count, key, count);
    const bool occ = key != FIN_LINK_EMPTY;
    const ull tr = fin_wave_sum64(occ ? count : 0ull);
    const uint32_t self = (uint32_t)__popcll(__ballot(occ && (uint32_t)(key >> 32) == (uint32_t)key));
    if ((threadIdx.x & 63u) == 0u) {
        if (tr) (void)__hip_atomic_fetch_add(stats, tr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (self) (void)__hip_atomic_fetch_add(stats + 1, (ull)self, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint32_t n = fin_block_sum4(keep ? 1u : 0u, lds_w);
    if (threadIdx.x == 0) blk_sum[blockIdx.x] = n;
}

// out[blk_off[block] + the kept slots of the block before this thread] = the slot's link
__global__ __launch_bounds__(256) void fin_links_write_kernel(const ull* tab, uint32_t cap, ull min_count, const uint64_t* blk_off, const uint32_t* ends_p, uint32_t n_unitigs,
                                                              LinkOut* out) {
    __shared__ uint32_t lds_w[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    ull key, count;
    const bool keep = links_slot(tab, cap, blockIdx.x * FIN_LINKS_BLK + threadIdx.x, min_count, key, count);
    const ull m = __ballot(keep);
    if (lane == 0u) lds_w[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!keep) return;
    uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t q = 0; q < wave; q++) before += lds_w[q];
    const uint32_t ga = (uint32_t)(key >> 32), gb = (uint32_t)key;
    const uint32_t ua = links_unitig_of(ends_p, n_unitigs, ga), ub = links_unitig_of(ends_p, n_unitigs, gb);
    out[blk_off[blockIdx.x] + before] = LinkOut{ua, ga - ends_p[ua], ub, gb - ends_p[ub], count};
}

extern "C" uint32_t fin_links_blocks(uint32_t cap) { return (cap + FIN_LINKS_BLK - 1u) / FIN_LINKS_BLK; }

extern "C" int fin_launch_links_clear(void* tab, uint32_t cap, hipStream_t stream) {
    if (cap < 4u || (cap & (cap - 1u))) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fin_links_clear_kernel, dim3(fin_links_blocks(cap)), dim3(256), 0, stream, (ull*)tab, cap);
    return (int)hipGetLastError();
}

extern "C" int fin_launch_links_add(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, const uint32_t* ends_p, uint32_t n_unitigs,
                                    uint64_t total_len, void* tab, uint32_t cap, uint64_t max_links, const uint32_t* ovf_count, uint32_t ovf_cap, hipStream_t stream) {
    if (n_reads == 0) return 0;
    if (cap < 4u || (cap & (cap - 1u))) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fin_links_add_kernel, dim3((n_reads + 255u) / 256u), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs, n_reads, ends_p,
                       n_unitigs, total_len, (ull*)tab, cap, (ull)max_links, ovf_count, ovf_cap);
    return (int)hipGetLastError();
}

extern "C" int fin_launch_links_count(const void* tab, uint32_t cap, uint64_t min_count, uint32_t* blk_sum, uint64_t* blk_off, uint64_t* total, uint64_t* stats,
                                      hipStream_t stream) {
    const uint32_t nb = fin_links_blocks(cap);
    hipLaunchKernelGGL(fin_links_count_kernel, dim3(nb), dim3(256), 0, stream, (const ull*)tab, cap, (ull)min_count, blk_sum, (ull*)stats);
    return fin_launch_blk_scan(blk_sum, nb, blk_off, total, stream);
}

extern "C" int fin_launch_links_write(const void* tab, uint32_t cap, uint64_t min_count, const uint64_t* blk_off, const uint32_t* ends_p, uint32_t n_unitigs, void* out,
                                      hipStream_t stream) {
    if (n_unitigs == 0) return 0;
    hipLaunchKernelGGL(fin_links_write_kernel, dim3(fin_links_blocks(cap)), dim3(256), 0, stream, (const ull*)tab, cap, (ull)min_count, blk_off, ends_p, n_unitigs,
                       (LinkOut*)out);
    return (int)hipGetLastError();
}
