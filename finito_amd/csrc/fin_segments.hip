// fin_segments.hip -- a batch's results as SEGMENTS: per read, the straight stretches its found slots make inside a unitig (include/finito_amd.h: fin_segment,
// fin_batch_segments).  A segment {u, off, slot, len} says that output slots slot .. slot + |len| - 1 of the read were found in unitig u, slot
// slot + j at offset off + j (len > 0) or off - j (len < 0).  The output is dense and in read order: seg_offs[n_reads + 1] (uint64, CSR) and the segments.
//
// The rule (canonical and local -- three neighbouring slots decide, no scan over the read).  link(i) = +1 / -1 when slots i - 1 and i are both found, in the same
// unitig, and off[i] - off[i - 1] is +1 / -1; 0 otherwise, and link(0) = 0.  A found slot i is a segment HEAD when link(i) = 0, or when link(i - 1) is neither
// 0 nor link(i).  A segment runs from its head to the slot before the next head or the next absent slot; its direction is the sign of its internal links (+ for
// a single slot).  Offsets 5,6,5,6,5 in one unitig give [5,6] [5] [6] [5].  This is NOT fin_cover_rec_kernel's run rule (that one merges greedily, a bitmap
// does not care where a run is cut).
//
// What is read (the frame is fin_wave.h's).  Where the step left records, a lane per read:
//   kind 1 -- at most nine found stretches (sgm_rec_walk), each one segment.  A read found on its reverse strand (meta bit 8) has output slot i = strand slot
//             nk - 1 - i: its stretches come out in reverse order, `off` at the stretch's highest offset, len < 0.
//   kind 0 -- the wave scans the read's pairs, a row of 64 slots at a time, the next row loaded ahead: links from neighbour compares, heads from the rule
//             (fin_seg_head), a ballot.  The two-slot history (the last slot of the row before, and its link) is carried across rows in wave-uniform registers.
//             A head lane writes its segment; a segment still open at a row's end gets its u, off and slot from its head lane and its length from the row that
//             closes it, so every byte is written once.
//
// Three steps, because the output is dense: (1) fin_sgm_kernel<false> counts per read (cnt[r]) and per block of 256 reads; (2) the one-block scan
// (fin_launch_blk_scan, fin_records.hip) makes the blocks' exclusive prefix and the total in uint64; (3) fin_sgm_kernel<true> scans its block's counts, writes seg_offs and the segments.  The kind-0
// pairs are read twice.  Records, pairs and text are read only; plain vector stores only.
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_wave.h"

#define FIN_SGM_BLK 256u   // reads per block: a lane per read

namespace {
typedef unsigned long long ull;

// slots [lo, hi) of the pair array are one read's: its segments counted (WRITE false) or written to out[0 ..) (WRITE true), the whole wave, a row of 64 slots
// at a time.  Wave-converged; returns the read's number of segments in every lane.
template <bool WRITE>
__device__ __forceinline__ uint32_t sgm_scan(const int2* pairs, uint64_t lo, uint64_t hi, uint4* out) {
    const uint32_t lane = threadIdx.x & 63u;
    FinSegCarry carry;
    uint32_t cnt = 0;
    bool open = false;                      // a segment reached the end of the row before: its ordinal, its slots so far, its direction (0: not known yet)
    uint32_t open_idx = 0, open_len = 0;
    int open_dir = 0;
    fin_each_pair_row(pairs, lo, hi, [&](uint64_t base, uint64_t j, int2 p) {
        const bool last_row = base + 64u >= hi;
        const uint32_t u = (uint32_t)p.x, off = (uint32_t)p.y;
        const bool found = u != 0xFFFFFFFFu;   // (an inactive lane holds (-1,-1))
        int link;
        const bool head = fin_seg_head(u, off, found, carry, link);
        const ull H = __ballot(head);
        if (WRITE) {
            const ull B = __ballot(head || !found);   // where a segment ends: the next head, the next absent slot, the read's end
            const ull PD = __ballot(link == -1);
            if (open) {
                const uint32_t b = B ? (uint32_t)__ffsll((long long)B) - 1u : 64u;   // slots of this row that continue it
                if (b > 0u && open_dir == 0) open_dir = (PD & 1ull) ? -1 : 1;
                open_len += b;
                if (b < 64u || last_row) {
                    if (lane == 0u) ((int*)(out + open_idx))[3] = open_dir < 0 ? -(int)open_len : (int)open_len;
                    open = false;
                }
            }
            if (head) {
                const ull above = lane == 63u ? 0ull : (B >> (lane + 1u)) << (lane + 1u);
                const uint32_t end = above ? (uint32_t)__ffsll((long long)above) - 1u : 64u;
                const uint32_t n = end - lane;   // 1 .. 64
                const bool down = n > 1u && ((PD >> (lane + 1u)) & 1ull);
                const uint32_t idx = cnt + (uint32_t)__popcll(H & ((1ull << lane) - 1ull));
                if (end == 64u && !last_row) {   // open: the closing row writes len
                    uint32_t* const w = (uint32_t*)(out + idx);
                    w[0] = u; w[1] = off; w[2] = (uint32_t)(j - lo);
                } else out[idx] = make_uint4(u, off, (uint32_t)(j - lo), (uint32_t)(down ? -(int)n : (int)n));
            }
            if (H && !last_row) {
                const uint32_t hl = 63u - (uint32_t)__clzll((long long)H);
                if ((hl == 63u ? 0ull : B >> (hl + 1u)) == 0ull) {
                    open = true; open_idx = cnt + (uint32_t)__popcll(H) - 1u; open_len = 64u - hl;
                    open_dir = open_len > 1u ? (((PD >> (hl + 1u)) & 1ull) ? -1 : 1) : 0;
                }
            }
        }
        cnt += (uint32_t)__popcll(H);
        fin_seg_next_row(carry, u, off, link);
    });
    return cnt;
}
}  // namespace

// WRITE false: cnt[r] = read r's number of segments, blk_sum[block] their sum over the block's reads.
// WRITE true:  seg_offs[r] = blk_off[block] + the exclusive prefix of cnt[] inside the block, seg_offs[n_reads] the total; the segments.
// frec null: the step left no records, every read is scanned.
template <bool WRITE>
__global__ __launch_bounds__(256) void fin_sgm_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_reads, uint32_t k, uint32_t* cnt,
                                                      uint32_t* blk_sum, const uint64_t* blk_off, uint64_t* seg_offs, uint4* segs) {
    __shared__ uint32_t lds_w[4];
    const uint32_t r = blockIdx.x * FIN_SGM_BLK + threadIdx.x;
    const FinReadItem it = fin_read_item<true>(frec, out_offs, r, n_reads);
    uint32_t mine = 0;
    uint64_t at = 0;   // WRITE: where this read's segments begin
    if (WRITE) {
        if (r < n_reads) mine = cnt[r];
        at = blk_off[blockIdx.x] + fin_block_exclusive4(mine, lds_w, nullptr);
        if (r < n_reads) seg_offs[r] = at;
        if (r == n_reads - 1u) seg_offs[n_reads] = at + mine;
    }
    if (it.kind == 1u && it.a.w != 0u) {
        const uint4 a = it.a, b = it.b;
        if (WRITE) {
            const bool rev = (a.z >> 8) & 1u;
            uint4* const out = segs + at;
            (void)sgm_rec_walk(a, b, k, [&](uint32_t s, uint32_t from, uint32_t to) {
                const uint32_t n = to - from;
                if (!rev) out[s] = make_uint4(a.x, a.y + from, from, n);
                else out[mine - 1u - s] = make_uint4(a.x, a.y + to - 1u, a.w - to, (uint32_t)(n == 1u ? 1 : -(int)n));
            });
        } else mine = sgm_rec_walk(a, b, k, [](uint32_t, uint32_t, uint32_t) {});
    }
    fin_each_searched_read(it, [&](int src, uint64_t lo, uint64_t hi) {
        const uint32_t c = sgm_scan<WRITE>(pairs, lo, hi, segs + fin_bcast64(at, src));
        if (!WRITE && (int)(threadIdx.x & 63u) == src) mine = c;
    });
    if (!WRITE) {
        if (r < n_reads) cnt[r] = mine;
        const uint32_t s = fin_block_sum4(mine, lds_w);
        if (threadIdx.x == 0) blk_sum[blockIdx.x] = s;
    }
}

extern "C" uint32_t fin_sgm_blocks(uint32_t n_reads) { return (n_reads + FIN_SGM_BLK - 1u) / FIN_SGM_BLK; }
// cnt: n_reads u32; blk_sum: fin_sgm_blocks() u32; blk_off: as many u64; total: one u64 (the batch's segments).  The counting pass and the scan.  n_reads > 0
extern "C" int fin_launch_sgm_count(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, uint32_t* cnt, uint32_t* blk_sum,
                                    uint64_t* blk_off, uint64_t* total, hipStream_t stream) {
    const uint32_t nb = fin_sgm_blocks(n_reads);
    if (nb == 0) return (int)hipMemsetAsync(total, 0, 8, stream);
    hipLaunchKernelGGL(fin_sgm_kernel<false>, dim3(nb), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs, n_reads, k, cnt, blk_sum,
                       (const uint64_t*)nullptr, (uint64_t*)nullptr, (uint4*)nullptr);
    return fin_launch_blk_scan(blk_sum, nb, blk_off, total, stream);
}
// seg_offs: n_reads + 1 u64; segs: room for *total segments of 16 bytes
extern "C" int fin_launch_sgm_write(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, const uint32_t* cnt,
                                    const uint64_t* blk_off, uint64_t* seg_offs, void* segs, hipStream_t stream) {
    const uint32_t nb = fin_sgm_blocks(n_reads);
    if (nb == 0) return (int)hipMemsetAsync(seg_offs, 0, 8, stream);
    hipLaunchKernelGGL(fin_sgm_kernel<true>, dim3(nb), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs, n_reads, k, (uint32_t*)cnt,
                       (uint32_t*)nullptr, blk_off, seg_offs, (uint4*)segs);
    return (int)hipGetLastError();
}
