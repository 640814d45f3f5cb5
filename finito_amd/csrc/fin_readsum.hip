// fin_readsum.hip -- a batch's results as one SUMMARY per read, and a SCREEN of the reads made from the summaries (include/finito_amd.h: fin_read_summary,
// fin_batch_read_summaries, fin_batch_screen).  The per-read counterpart of fin_hits.hip: which reads belong to the reference, and how well.
//
// The summary {n_found, n_segments, longest, span} is defined over the read's output slots 0 .. nk - 1 (fin_search_batch's pairs): the found slots, the segments
// under the rule of fin_segments.hip (link(i) and link(i - 1) decide a head), the longest segment, and last found slot - first found slot + 1.  All four are the
// same when the slot order is reversed, so a record found on the reverse strand (meta bit 8) needs no special case.
//
// What is read (the frame is fin_wave.h's).  Where the step left records, a lane per read:
//   kind 1 -- through sgm_rec_walk: n_found = the sum of the stretches, n_segments = how many, longest = the longest, span = the last stretch's end - the first
//             one's start.
//   kind 2 -- all zero.
//   kind 0 -- the wave scans the read's pairs, a row of 64 slots at a time, the next row loaded ahead.  Links and heads by fin_seg_head; found slots and heads are
//             counted from ballots.  Carried across rows, in wave-uniform registers: the two-slot history of the head rule, the length so far of the segment
//             still open at the row's end (so `longest` is right for a segment that crosses any number of rows), the first and the last found slot.
// A lane writes its read's summary as one 16-byte store; nothing else is written, and there are no atomics: every output word has one writer.
//
// The screen: read r passes when (n_found >= min_found && 1000 * n_found >= min_permille * nk) != invert, in 64-bit arithmetic, nk from out_offs.  bits: a
// wave's ballot is one uint64 word of the bitmap, stored by lane 0.  ids: the passing read numbers, dense and ascending, by the three steps of fin_sgm_*: (1)
// fin_scr_bits_kernel also counts per block of 256 reads, (2) the one-block uint64 scan (fin_launch_blk_scan, fin_records.hip), (3) fin_scr_ids_kernel
// places a read at its block's offset + the passing reads before it in the block, taken from the bitmap's words.
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_wave.h"

#define FIN_RSM_BLK 256u   // reads per block: a lane per read

namespace {
typedef unsigned long long ull;

// slots [lo, hi) of the pair array are one read's: its summary {n_found, n_segments, longest, span}, the whole wave, a row of 64 slots at a time.
// Wave-converged; every lane returns the same value.
__device__ __forceinline__ uint4 rsm_scan(const int2* pairs, uint64_t lo, uint64_t hi) {
    const uint32_t lane = threadIdx.x & 63u;
    FinSegCarry carry;
    uint32_t n_found = 0, n_seg = 0, longest = 0;
    uint32_t open_len = 0;                  // a segment reached the end of the row before: its slots so far (0: none did)
    uint32_t first = 0xFFFFFFFFu, last = 0; // the first and the last found slot so far
    fin_each_pair_row(pairs, lo, hi, [&](uint64_t base, uint64_t, int2 p) {
        const uint32_t u = (uint32_t)p.x, off = (uint32_t)p.y;
        const bool found = u != 0xFFFFFFFFu;
        int link;
        const bool head = fin_seg_head(u, off, found, carry, link);
        const ull F = __ballot(found), H = __ballot(head);
        const ull B = H | ~F;               // where a segment ends: the next head, the next absent slot (a lane beyond the read's end is one)
        n_found += (uint32_t)__popcll(F);
        n_seg += (uint32_t)__popcll(H);
        if (F) {
            const uint32_t row = (uint32_t)(base - lo);
            if (first == 0xFFFFFFFFu) first = row + (uint32_t)__ffsll((long long)F) - 1u;
            last = row + 63u - (uint32_t)__clzll((long long)F);
        }
        if (open_len) {                     // the segment that came in: the slots of this row that continue it
            const uint32_t b = B ? (uint32_t)__ffsll((long long)B) - 1u : 64u;
            open_len += b;
            if (b < 64u) { longest = max(longest, open_len); open_len = 0; }
        }
        if (H) {                            // the segments that begin in this row (a head closes whatever came in: open_len is 0 here)
            const ull above = lane == 63u ? 0ull : (B >> (lane + 1u)) << (lane + 1u);
            const uint32_t end = above ? (uint32_t)__ffsll((long long)above) - 1u : 64u;
            // closed inside the row; the one that reaches the row's end (the last head's, if any) stays open
            longest = max(longest, fin_wave_max(head && end < 64u ? end - lane : 0u));
            const uint32_t hl = 63u - (uint32_t)__clzll((long long)H);
            if ((hl == 63u ? 0ull : B >> (hl + 1u)) == 0ull) open_len = 64u - hl;
        }
        fin_seg_next_row(carry, u, off, link);
    });
    longest = max(longest, open_len);       // (the read ended on a row's last slot)
    return make_uint4(n_found, n_seg, longest, n_found ? last - first + 1u : 0u);
}
}  // namespace

// sum[r] = read r's summary.  frec null: the step left no records, every read is scanned.
__global__ __launch_bounds__(256) void fin_rsm_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, uint32_t n_reads, uint32_t k, uint4* sum) {
    const uint32_t r = blockIdx.x * FIN_RSM_BLK + threadIdx.x, lane = threadIdx.x & 63u;
    const FinReadItem it = fin_read_item<true>(frec, out_offs, r, n_reads);
    uint4 mine = make_uint4(0u, 0u, 0u, 0u);
    if (it.kind == 1u && it.a.w != 0u) {
        uint32_t n_found = 0, longest = 0, first = 0, last = 0;
        const uint32_t n = sgm_rec_walk(it.a, it.b, k, [&](uint32_t s, uint32_t from, uint32_t to) {
            n_found += to - from; longest = max(longest, to - from);
            if (s == 0u) first = from;
            last = to;
        });
        mine = make_uint4(n_found, n, longest, last - first);   // (no stretch: first = last = 0)
    }
    fin_each_searched_read(it, [&](int src, uint64_t lo, uint64_t hi) {
        const uint4 s = rsm_scan(pairs, lo, hi);
        if ((int)lane == src) mine = s;
    });
    if (r < n_reads) sum[r] = mine;
}

// bits[w] = the ballot of "read 64 w + lane passes"; blk_sum[block] = how many of the block's reads pass.  A lane beyond n_reads does not pass
__global__ __launch_bounds__(256) void fin_scr_bits_kernel(const uint4* sum, const uint64_t* out_offs, uint32_t n_reads, uint32_t min_found, uint32_t min_permille,
                                                           uint32_t invert, uint64_t* bits, uint32_t* blk_sum) {
    __shared__ uint32_t lds_w[4];
    const uint32_t r = blockIdx.x * FIN_RSM_BLK + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool pass = false;
    if (r < n_reads) {
        const uint64_t nf = sum[r].x, nk = out_offs[r + 1] - out_offs[r];
        pass = (nf >= (uint64_t)min_found && 1000ull * nf >= (uint64_t)min_permille * nk) != (invert != 0u);
    }
    const ull w = __ballot(pass);
    const uint32_t word = blockIdx.x * 4u + wave;
    if (lane == 0u) {
        if (word < (n_reads + 63u) / 64u) bits[word] = w;
        lds_w[wave] = (uint32_t)__popcll(w);
    }
    __syncthreads();
    if (threadIdx.x == 0) blk_sum[blockIdx.x] = lds_w[0] + lds_w[1] + lds_w[2] + lds_w[3];
}

// ids[blk_off[block] + the passing reads before r in its block] = r for every passing read r: ascending, dense
__global__ __launch_bounds__(256) void fin_scr_ids_kernel(const uint64_t* bits, const uint64_t* blk_off, uint32_t n_reads, uint32_t* ids) {
    const uint32_t r = blockIdx.x * FIN_RSM_BLK + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t word = blockIdx.x * 4u + wave, n_words = (n_reads + 63u) / 64u;
    if (word >= n_words) return;
    const uint64_t w = bits[word];
    if (!((w >> lane) & 1ull)) return;      // (bits at and beyond n_reads are 0)
    uint32_t before = (uint32_t)__popcll(w & ((1ull << lane) - 1ull));
    for (uint32_t q = 0; q < wave; q++) before += (uint32_t)__popcll(bits[blockIdx.x * 4u + q]);
    ids[blk_off[blockIdx.x] + before] = r;
}

extern "C" uint32_t fin_rsm_blocks(uint32_t n_reads) { return (n_reads + FIN_RSM_BLK - 1u) / FIN_RSM_BLK; }
extern "C" int fin_launch_read_summaries(const void* frec, const uint64_t* out_offs, const void* pairs, uint32_t n_reads, uint32_t k, void* sum, hipStream_t stream) {
    const uint32_t nb = fin_rsm_blocks(n_reads);
    if (nb == 0) return 0;
    hipLaunchKernelGGL(fin_rsm_kernel, dim3(nb), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs, n_reads, k, (uint4*)sum);
    return (int)hipGetLastError();
}
extern "C" int fin_launch_screen_bits(const void* sum, const uint64_t* out_offs, uint32_t n_reads, uint32_t min_found, uint32_t min_permille, int invert,
                                      uint64_t* bits, uint32_t* blk_sum, uint64_t* blk_off, uint64_t* total, hipStream_t stream) {
    const uint32_t nb = fin_rsm_blocks(n_reads);
    if (nb == 0) return (int)hipMemsetAsync(total, 0, 8, stream);
    hipLaunchKernelGGL(fin_scr_bits_kernel, dim3(nb), dim3(256), 0, stream, (const uint4*)sum, out_offs, n_reads, min_found, min_permille, invert ? 1u : 0u, bits, blk_sum);
    return fin_launch_blk_scan(blk_sum, nb, blk_off, total, stream);
}
extern "C" int fin_launch_screen_ids(const uint64_t* bits, const uint64_t* blk_off, uint32_t n_reads, uint32_t* ids, hipStream_t stream) {
    const uint32_t nb = fin_rsm_blocks(n_reads);
    if (nb == 0) return 0;
    hipLaunchKernelGGL(fin_scr_ids_kernel, dim3(nb), dim3(256), 0, stream, bits, blk_off, n_reads, ids);
    return (int)hipGetLastError();
}
