// fin_pileup.hip -- a run's base PILEUP over the unitig set: per position g of the concatenated unitig text, how many placed reads span it (cover) and how many
// show each base other than the text's (alt), and the CALL made from both: the positions where the sample differs from the indexed sequence
// (include/finito_amd.h: fin_pileup, fin_batch_add_pileup, fin_pileup_call).  The siblings answer where a read's k-mers lie; this file answers
// what the read says there.  The geometry is fin_depth's: start(u) = ends_p[u], total_len positions.
//
// The definition, on the pairs fin_search_batch delivers (every producer must agree with it).  A read of L bases, nk = L - k + 1 slots:
//   straight -- at least two found slots, all in one unitig u, and off - i is one constant dF over them (forward) or off + i one constant dR (reverse);
//   placed   -- strand A (the read forward, or its reverse complement) lies at offsets [s0, s0 + L) of u, s0 = dF or dR - nk + 1, all of them inside u;
//   mismatch -- a strand-A base that is A, C, G or T (either case) and differs from the text's; any other letter is no observation.  More than max_mismatch
//               mismatches drop the read whole;
//   a kept read adds +1 to cover at each of its L positions and +1 to alt[g][b] at each mismatch, b the observed code in the text's orientation.
// Four counters: kept, not straight (reads shorter than k among them), straight but not inside the unitig, dropped for too many mismatches.
//
// The accumulator: uint32 alt[total_len][4], a 16-byte line per position; the counters (4 x u64); the flag word (bit 0: a withheld step was offered -- nothing of
// it is added; bit 1: a slot or record outside the index -- the read counts as not straight, a record as not inside its unitig); and cover as fin_depth.hip's
// DIFFERENCE array, int32 cov_diff[total_len + 1]: two adds per kept read, both ends known to be valid before either is issued (a read is placed only inside its
// unitig, and the unitig inside the text).  Adds are relaxed, agent-scope __hip_atomic_fetch_add, result unused: integer adds commute, the result is exact
// whatever order the lanes arrive in, and a run added twice counts twice.  Modulo 2^32.  No waiting, no floating point.
//
// What is read (the frame is fin_wave.h's): the step's records and pairs, the batch's ASCII bases (bases, offs -- still resident behind the step) and the
// replica's 2-bit text.
//   kind 1 -- the record alone: place and direction (meta bit 8), the found slots from the stretches of fin_rec_walk.h, nE = meta & 0xFF against max_mismatch;
//             one alt add per disagreeing position E: the strand's base there is read[E] forward, the complement of read[L - 1 - E] reverse.  The fast path puts
//             only ACGT reads into records and lists every position whose code differs from the text's (fin_prepass.hip: fast_try), so the positions ARE the
//             read's mismatches; the text is not read.  Pairs are never touched.
//   kind 0 -- the wave takes the read.  Pass 1 scans its pair rows: the first found slot's u, dF and dR and the found count, wave-uniform, a ballot per row for
//             "every found lane agrees" on each diagonal.  Pass 2, only for a read that is straight and inside its unitig: 64 bases per row, lane j a base,
//             against the text; popcounts of the mismatch ballot are summed.  Pass 3, only within max_mismatch: the same rows again, a lane per mismatching
//             base adds to alt, lane 0 issues the two cover adds.  Nothing is indexed by a run-time count: no scratch.
//
// On a set that is not disjoint the same rule applies to the place the reference reports: exact against the model, but a read may be compared with a place that
// does not spell it (as depth and cover count a k-mer in the copy that is the reference's choice).
//
// The call: per chunk of staged cover (fin_launch_depth_scan_chunk's output), a counting pass (a block counts the candidates among its 256 positions), the
// one-block scan of the counts (fin_launch_blk_scan) and a writing pass that stores the entries ascending.  No block waits for another.
//
// Out of scope: partitioned indexes, fin_search_batch_multi / dist.py, the C++ mirror, indels, base qualities, saturation, reads that bridge unitigs.
#include "fin_device.h"
#include "fin_kernels.h"
#include "fin_wave.h"

namespace {
typedef unsigned long long ull;

__device__ __forceinline__ void pile_flag(uint32_t* flags, uint32_t bit) { (void)__hip_atomic_fetch_or(flags, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void pile_alt(uint32_t* alt, uint64_t g, uint32_t b) {
    (void)__hip_atomic_fetch_add(alt + g * 4u + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// positions [g_lo, g_end) each covered once more.  The caller has checked g_lo < g_end <= total_len
__device__ __forceinline__ void pile_cover(int32_t* diff, uint64_t g_lo, uint64_t g_end) {
    (void)__hip_atomic_fetch_add(diff + g_lo, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(diff + g_end, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// A, C, G, T in either case -> 0 .. 3; anything else -> 4: no observation
__device__ __forceinline__ uint32_t pile_code(uint32_t ch) {
    const uint32_t x = ch & 0xDFu;
    return x == 'A' ? 0u : x == 'C' ? 1u : x == 'G' ? 2u : x == 'T' ? 3u : 4u;
}
__device__ __forceinline__ uint32_t pile_text(const uint32_t* concat, uint64_t g) { return (concat[g >> 4] >> (2u * ((uint32_t)g & 15u))) & 3u; }

// the outcomes a read can have: the counters' order
enum : uint32_t { PILE_KEPT = 0u, PILE_NOT_STRAIGHT = 1u, PILE_OFF_UNITIG = 2u, PILE_TOO_MANY = 3u, PILE_NONE = 4u };

// a kind-0 read, the whole wave: slots [lo, hi) of the pair array, its bases at bases[b0 ..).  Wave-converged; returns the read's outcome
__device__ __forceinline__ uint32_t pile_searched(const int2* pairs, uint64_t lo, uint64_t hi, const uint8_t* bases, uint64_t b0, uint32_t k, const uint32_t* ends_p,
                                                  const uint32_t* concat, uint32_t n_unitigs, uint64_t total_len, uint32_t max_mm, uint32_t* alt, int32_t* diff,
                                                  uint32_t* flags) {
    const uint32_t lane = threadIdx.x & 63u;
    // ---- pass 1: is the read straight? ----
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
    if (outside) { if (lane == 0u) pile_flag(flags, 2u); return PILE_NOT_STRAIGHT; }
    if (n_found < 2u || okF == okR) return PILE_NOT_STRAIGHT;   // (with two found slots both diagonals cannot hold; neither: a mosaic, an indel, a repeated pair)
    // ---- placed: strand A at offsets [s0, s0 + L) of u0 ----
    const uint32_t nk = (uint32_t)(hi - lo), L = nk + k - 1u;
    const bool rev = okR;
    const int64_t s0 = rev ? (int64_t)dR - (int64_t)nk + 1 : (int64_t)dF;
    const uint64_t ustart = ends_p[u0], uend = ends_p[u0 + 1u];
    if (s0 < 0 || ustart + (uint64_t)s0 + L > uend || uend > total_len) return PILE_OFF_UNITIG;
    const uint64_t g0 = ustart + (uint64_t)s0;
    // ---- passes 2 and 3: the read against the text, 64 bases a row; lane j's base p lies at strand position s ----
    uint32_t n_mm = 0;
    for (uint32_t pass = 2u; pass <= 3u; pass++) {
        for (uint32_t jb = 0; jb < L; jb += 64u) {
            const uint32_t p = jb + lane;
            bool mm = false;
            uint32_t obs = 4u;
            uint64_t g = 0;
            if (p < L) {
                const uint32_t c = pile_code(bases[b0 + p]);
                obs = rev && c < 4u ? 3u - c : c;
                g = g0 + (rev ? L - 1u - p : p);
                mm = obs < 4u && obs != pile_text(concat, g);
            }
            if (pass == 2u) n_mm += (uint32_t)__popcll(__ballot(mm));
            else if (mm) pile_alt(alt, g, obs);
        }
        if (pass == 2u && n_mm > max_mm) return PILE_TOO_MANY;
    }
    if (lane == 0u) pile_cover(diff, g0, g0 + L);
    return PILE_KEPT;
}

// the unitig of text position g: the last u in [0, n_unitigs) with ends_p[u] <= g (ends_p[0] = 0)
__device__ __forceinline__ uint32_t pile_unitig_of(const uint32_t* ends_p, uint32_t n_unitigs, uint64_t g) {
    uint32_t lo = 0, hi = n_unitigs;
    while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if ((uint64_t)ends_p[mid] <= g) lo = mid; else hi = mid; }
    return lo;
}
// position i of the staged chunk: a candidate?  a = its alt line
__device__ __forceinline__ bool pile_candidate(const uint32_t* cover, const uint4* alt, uint64_t i, uint64_t n, uint32_t min_alt, uint32_t min_permille, uint4& a, uint32_t& cov) {
    if (i >= n) return false;
    a = alt[i]; cov = cover[i];
    const uint32_t m = max(max(a.x, a.y), max(a.z, a.w));
    return m >= max(min_alt, 1u) && 1000ull * m >= (ull)min_permille * cov;
}
}  // namespace

// A lane per read; the wave takes its lanes' searched reads in turn.  frec null: every read is kind 0
__global__ __launch_bounds__(256) void fin_pileup_add_kernel(const FinFastRec* frec, const uint64_t* out_offs, const int2* pairs, const uint8_t* bases, const uint64_t* offs,
                                                             uint32_t n_reads, uint32_t k, const uint32_t* ends_p, const uint32_t* concat, uint32_t n_unitigs,
                                                             uint64_t total_len, uint32_t max_mm, uint32_t* alt, int32_t* diff, ull* counters, uint32_t* flags,
                                                             const uint32_t* ovf_count, uint32_t ovf_cap) {
    if (fin_step_withheld(ovf_count, ovf_cap, flags)) return;
    const uint32_t r = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const FinReadItem it = fin_read_item<false>(frec, out_offs, r, n_reads);
    uint32_t outcome = r < n_reads ? PILE_NOT_STRAIGHT : PILE_NONE;   // (kind 2, a read shorter than k: no found slot)
    uint64_t b0 = 0;
    if (r < n_reads && (it.kind == 1u || it.scanned())) b0 = offs[r];
    if (it.kind == 1u && it.a.w != 0u) {
        const uint4 a = it.a;
        const uint32_t nk = a.w, L = nk + k - 1u, nE = a.z & 0xFFu;
        const bool rev = (a.z >> 8) & 1u;
        // u and the extent against the unitig's bounds before any add
        uint64_t ustart = 0, uend = 0;
        if (a.x < n_unitigs) { ustart = ends_p[a.x]; uend = ends_p[a.x + 1u]; }
        if (a.x >= n_unitigs || ustart + a.y + L > uend || uend > total_len) { pile_flag(flags, 2u); outcome = PILE_OFF_UNITIG; }
        else {
            const uint4 b = it.load_b();
            uint32_t n_found = 0;
            (void)sgm_rec_walk(a, b, k, [&](uint32_t, uint32_t from, uint32_t to) { n_found += to - from; });
            if (n_found < 2u) outcome = PILE_NOT_STRAIGHT;
            else if (nE > max_mm) outcome = PILE_TOO_MANY;
            else {
                const uint64_t g0 = ustart + a.y;
#pragma unroll
                for (uint32_t e = 0; e < 8u; e++) {
                    if (e < nE) {
                        const uint32_t w = e < 2u ? b.x : e < 4u ? b.y : e < 6u ? b.z : b.w, E = (e & 1u) ? w >> 16 : w & 0xFFFFu;
                        if (E < L) {
                            const uint32_t c = pile_code(bases[b0 + (rev ? L - 1u - E : E)]);
                            if (c < 4u) pile_alt(alt, g0 + E, rev ? 3u - c : c);
                        } else pile_flag(flags, 2u);
                    }
                }
                pile_cover(diff, g0, g0 + L);
                outcome = PILE_KEPT;
            }
        }
    }
    fin_each_searched_read(it, [&](int src, uint64_t lo, uint64_t hi) {
        const uint32_t o = pile_searched(pairs, lo, hi, bases, fin_bcast64(b0, src), k, ends_p, concat, n_unitigs, total_len, max_mm, alt, diff, flags);
        if ((int)lane == src) outcome = o;
    });
    // the counters: a wave's reads by outcome, one add each
#pragma unroll
    for (uint32_t c = 0; c < 4u; c++) {
        const ull n = (ull)__popcll(__ballot(outcome == c));
        if (n && lane == 0u) (void)__hip_atomic_fetch_add(counters + c, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the call over one staged chunk: cover[0 .. n) and alt[0 .. n) are text positions g_base .. g_base + n ----
// 1. blk_sum[b] = the candidates among block b's 256 positions
__global__ __launch_bounds__(256) void fin_pileup_call_count_kernel(const uint32_t* cover, const uint4* alt, uint64_t n, uint32_t min_alt, uint32_t min_permille,
                                                                    uint32_t* blk_sum) {
    __shared__ uint32_t lds[4];
    uint4 a; uint32_t cov;
    const bool cand = pile_candidate(cover, alt, (uint64_t)blockIdx.x * 256u + threadIdx.x, n, min_alt, min_permille, a, cov);
    const uint32_t total = fin_block_sum4(cand ? 1u : 0u, lds);
    if (threadIdx.x == 0) blk_sum[blockIdx.x] = total;
}
// 2. (fin_launch_blk_scan)  3. the entries, ascending: out[blk_off[b] + the candidates of the block before this thread]
__global__ __launch_bounds__(256) void fin_pileup_call_write_kernel(const uint32_t* cover, const uint4* alt, uint64_t g_base, uint64_t n, uint32_t min_alt,
                                                                    uint32_t min_permille, const uint32_t* ends_p, const uint32_t* concat, uint32_t n_unitigs,
                                                                    const uint64_t* blk_off, uint4* out) {
    __shared__ uint32_t lds[4];
    uint4 a; uint32_t cov;
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool cand = pile_candidate(cover, alt, i, n, min_alt, min_permille, a, cov);
    const uint32_t before = fin_block_exclusive4(cand ? 1u : 0u, lds, nullptr);
    if (cand) {
        const uint64_t g = g_base + i, at = blk_off[blockIdx.x] + before;
        const uint32_t u = pile_unitig_of(ends_p, n_unitigs, g);
        out[2u * at] = make_uint4(u, (uint32_t)(g - ends_p[u]), cov, pile_text(concat, g));
        out[2u * at + 1u] = a;
    }
}

// alt: uint32[total_len][4]; diff: int32[total_len + 1]; counters: 4 x u64; flags: one u32.  frec null: every read is kind 0.  bases / offs: the batch's ASCII
// reads and their n_reads + 1 offsets.  ovf_count (may be null) / ovf_cap as fin_launch_depth_add
extern "C" int fin_launch_pileup_add(const void* frec, const uint64_t* out_offs, const void* pairs, const uint8_t* bases, const uint64_t* offs, uint32_t n_reads, uint32_t k,
                                     const uint32_t* ends_p, const uint32_t* concat, uint32_t n_unitigs, uint64_t total_len, uint32_t max_mismatch, void* alt, void* diff,
                                     void* counters, uint32_t* flags, const uint32_t* ovf_count, uint32_t ovf_cap, hipStream_t stream) {
    if (n_reads == 0) return 0;
    if (n_unitigs == 0 || total_len == 0 || k == 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fin_pileup_add_kernel, dim3((n_reads + 255u) / 256u), dim3(256), 0, stream, (const FinFastRec*)frec, out_offs, (const int2*)pairs, bases, offs, n_reads,
                       k, ends_p, concat, n_unitigs, total_len, max_mismatch, (uint32_t*)alt, (int32_t*)diff, (ull*)counters, flags, ovf_count, ovf_cap);
    return (int)hipGetLastError();
}

extern "C" uint32_t fin_pileup_call_blocks(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }

// the candidates of one chunk, n <= 2^32 - 256 positions: blk_sum / blk_off have fin_pileup_call_blocks(n) entries, *total their number
extern "C" int fin_launch_pileup_call_count(const uint32_t* cover, const void* alt, uint64_t n, uint32_t min_alt, uint32_t min_permille, uint32_t* blk_sum,
                                            uint64_t* blk_off, uint64_t* total, hipStream_t stream) {
    if (n == 0) return (int)hipErrorInvalidValue;
    const uint32_t n_blk = fin_pileup_call_blocks(n);
    hipLaunchKernelGGL(fin_pileup_call_count_kernel, dim3(n_blk), dim3(256), 0, stream, cover, (const uint4*)alt, n, min_alt, min_permille, blk_sum);
    const int rc = (int)hipGetLastError();
    return rc ? rc : fin_launch_blk_scan(blk_sum, n_blk, blk_off, total, stream);
}
// ... written to out, which has room for *total entries of 32 bytes
extern "C" int fin_launch_pileup_call_write(const uint32_t* cover, const void* alt, uint64_t g_base, uint64_t n, uint32_t min_alt, uint32_t min_permille,
                                            const uint32_t* ends_p, const uint32_t* concat, uint32_t n_unitigs, const uint64_t* blk_off, void* out, hipStream_t stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(fin_pileup_call_write_kernel, dim3(fin_pileup_call_blocks(n)), dim3(256), 0, stream, cover, (const uint4*)alt, g_base, n, min_alt, min_permille, ends_p,
                       concat, n_unitigs, blk_off, (uint4*)out);
    return (int)hipGetLastError();
}
