// fin_segments_check, fin_segments_window_depth and fin_segments_lift_variants (finito_amd/csrc/fin_refpaths_host.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer, as a stand-alone program: no Python, no device, no HIP.  From the repository root:
//   g++ -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=c++17 -fopenmp -o /tmp/asan_refpaths tools/asan_refpaths.cpp \
//       finito_amd/csrc/fin_refpaths_host.cpp finito_amd/csrc/fin_records_host.cpp finito_amd/csrc/fin_taxa_host.cpp
//   /tmp/asan_refpaths
// (fin_records_host.cpp provides fin_host_threads; its read-taxa twin calls fin_taxa_call and fin_taxa_first_bad_parent, which fin_taxa_host.cpp defines)
// 3000 hand-made sequences -- segments forward and reverse over four unitigs, touching both ends of their unitigs and of their sequences, sequences without slots and
// without segments --, windows 1, 7, 64 and 1000, one thread and seven; every buffer of exactly the size the header asks for; a variant at every position of the text;
// every refusal.  The expectation is worked out here, slot by slot and base by base.  It prints "ok" and exits 0 when the calls gave what they must and the
// sanitizers reported nothing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/finito_amd.h"

#define MUST(x) do { if (!(x)) { fprintf(stderr, "failed: %s (line %d, window = %u, threads = %d)\n", #x, __LINE__, window, threads); return 1; } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd64() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static uint32_t rnd(uint32_t n) { return (uint32_t)(rnd64() % n); }

static int run(uint32_t window, int threads) {
    const int k = 5;
    const std::vector<int64_t> lens = {3000, 90, 5, 40};
    std::vector<int64_t> ends, starts;
    int64_t total = 0;
    for (int64_t l : lens) { starts.push_back(total); total += l; ends.push_back(total); }
    const uint64_t n_seqs = 3000;
    std::vector<uint32_t> seq_nk(n_seqs);
    std::vector<uint64_t> seg_offs(n_seqs + 1, 0);
    std::vector<fin_segment> segs;
    for (uint64_t s = 0; s < n_seqs; s++) {
        const uint32_t nk = s % 11 == 0 ? 0u : 1u + rnd(400);
        seq_nk[s] = nk;
        uint32_t slot = 0;
        while (s % 7 != 0 && slot < nk) {
            slot += rnd(3);
            if (slot >= nk) break;
            const int32_t u = (int32_t)rnd(4);
            const uint32_t nku = (uint32_t)(lens[(size_t)u] - k + 1), room = nk - slot;
            const uint32_t n = 1u + rnd(nku < room ? nku : room);
            if (rnd(2)) segs.push_back(fin_segment{u, (int32_t)rnd(nku - n + 1u), slot, (int32_t)n});
            else segs.push_back(fin_segment{u, (int32_t)(n - 1u + rnd(nku - n + 1u)), slot, n == 1u ? 1 : -(int32_t)n});
            slot += n;
        }
        seg_offs[s + 1] = segs.size();
    }
    std::vector<uint32_t> depth((size_t)total);
    for (auto& d : depth) d = rnd(16) == 0 ? 0xFFFFFFFFu : rnd(5);
    char err[256] = {0};
    MUST(fin_segments_check(seq_nk.data(), seg_offs.data(), segs.data(), n_seqs, k, ends.data(), ends.size(), err, sizeof err) == FIN_OK);
    // ---- windows ----
    std::vector<uint64_t> wo(n_seqs + 1, 0);
    for (uint64_t s = 0; s < n_seqs; s++) wo[s + 1] = wo[s] + (seq_nk[s] + window - 1) / window;
    const uint64_t W = wo[n_seqs];
    std::vector<fin_ref_window> want(W, fin_ref_window{0, 0, 0});
    for (uint64_t s = 0; s < n_seqs; s++)
        for (uint64_t i = seg_offs[s]; i < seg_offs[s + 1]; i++) {
            const fin_segment& g = segs[i];
            const int64_t n = g.len < 0 ? -(int64_t)g.len : g.len;
            for (int64_t j = 0; j < n; j++) {
                const uint32_t d = depth[(size_t)(starts[(size_t)g.u] + g.off + (g.len > 0 ? j : -j))];
                fin_ref_window& o = want[(size_t)(wo[s] + (g.slot + (uint64_t)j) / window)];
                o.depth_sum += d; o.in_graph++; o.covered += d >= 3u;
            }
        }
    std::vector<uint64_t> got_wo(n_seqs + 1, 7);
    std::vector<fin_ref_window> got(W);   // exactly W
    uint64_t nw = 0;
    MUST(fin_segments_window_depth(seq_nk.data(), seg_offs.data(), segs.data(), n_seqs, k, ends.data(), ends.size(), depth.data(), window, 3, got_wo.data(), got.data(), W, &nw,
                                   threads, err, sizeof err) == FIN_OK);
    MUST(nw == W && got_wo == wo && memcmp(got.data(), want.data(), W * sizeof(fin_ref_window)) == 0);
    MUST(fin_segments_window_depth(seq_nk.data(), seg_offs.data(), segs.data(), n_seqs, k, ends.data(), ends.size(), depth.data(), window, 3, nullptr, got.data(), W - 1, &nw,
                                   threads, err, sizeof err) == FIN_ELIMIT && nw == W);
    MUST(fin_segments_window_depth(seq_nk.data(), seg_offs.data(), segs.data(), n_seqs, k, ends.data(), ends.size(), depth.data(), 0, 3, nullptr, got.data(), W, &nw, threads,
                                   err, sizeof err) == FIN_EINVAL);
    // ---- variants: one at every position of the text ----
    std::vector<fin_variant> vars((size_t)total);
    for (size_t u = 0, g = 0; u < lens.size(); u++)
        for (int64_t x = 0; x < lens[u]; x++, g++) { memset(&vars[g], 0, sizeof(fin_variant)); vars[g].u = (uint32_t)u; vars[g].off = (uint32_t)x; }
    std::vector<fin_ref_variant> wl;
    for (uint64_t s = 0; s < n_seqs; s++)
        for (uint64_t i = seg_offs[s]; i < seg_offs[s + 1]; i++) {
            const fin_segment& g = segs[i];
            const int64_t n = g.len < 0 ? -(int64_t)g.len : g.len;
            for (int64_t b = 0; b < n + k - 1; b++) {   // sequence base slot + b
                const int64_t x = g.len > 0 ? g.off + b : g.off + k - 1 - b;
                wl.push_back(fin_ref_variant{(uint32_t)s, (uint32_t)(g.slot + b), (uint32_t)(starts[(size_t)g.u] + x), g.len > 0 ? 0u : 1u});
            }
        }
    std::vector<fin_ref_variant> gl(wl.size());   // exactly as many
    uint64_t nl = 0;
    MUST(fin_segments_lift_variants(seq_nk.data(), seg_offs.data(), segs.data(), n_seqs, k, ends.data(), ends.size(), vars.data(), vars.size(), gl.data(), gl.size(), &nl,
                                    threads, err, sizeof err) == FIN_OK);
    MUST(nl == wl.size() && memcmp(gl.data(), wl.data(), wl.size() * sizeof(fin_ref_variant)) == 0);
    MUST(fin_segments_lift_variants(seq_nk.data(), seg_offs.data(), segs.data(), n_seqs, k, ends.data(), ends.size(), vars.data(), vars.size(), gl.data(), gl.size() - 1, &nl,
                                    threads, err, sizeof err) == FIN_ELIMIT && nl == wl.size());
    MUST(fin_segments_lift_variants(seq_nk.data(), seg_offs.data(), segs.data(), n_seqs, k, ends.data(), ends.size(), nullptr, 0, nullptr, 0, &nl, threads, err, sizeof err) ==
             FIN_OK && nl == 0);
    std::swap(vars[10], vars[11]);
    MUST(fin_segments_lift_variants(seq_nk.data(), seg_offs.data(), segs.data(), n_seqs, k, ends.data(), ends.size(), vars.data(), vars.size(), gl.data(), gl.size(), &nl,
                                    threads, err, sizeof err) == FIN_EINVAL && strstr(err, "ascend"));
    std::swap(vars[10], vars[11]);
    vars.back().off = (uint32_t)lens.back();
    MUST(fin_segments_lift_variants(seq_nk.data(), seg_offs.data(), segs.data(), n_seqs, k, ends.data(), ends.size(), vars.data(), vars.size(), gl.data(), gl.size(), &nl,
                                    threads, err, sizeof err) == FIN_EINVAL && strstr(err, "outside the index"));
    // ---- every clause of the validity rule, on the last segment ----
    const fin_segment keep = segs.back();
    const fin_segment bad[] = {{4, 0, keep.slot, 1}, {-1, 0, keep.slot, 1}, {keep.u, keep.off, keep.slot, 0}, {1, 0, keep.slot, 4000}, {1, 86, keep.slot, 1}, {1, -1, keep.slot, 1},
                               {1, 0, keep.slot, -2}, {1, 86, keep.slot, -2}};
    for (const fin_segment& b : bad) {
        segs.back() = b;
        MUST(fin_segments_check(seq_nk.data(), seg_offs.data(), segs.data(), n_seqs, k, ends.data(), ends.size(), err, sizeof err) == FIN_EINVAL && strstr(err, "segment"));
        MUST(fin_segments_window_depth(seq_nk.data(), seg_offs.data(), segs.data(), n_seqs, k, ends.data(), ends.size(), depth.data(), window, 3, nullptr, got.data(), W, &nw,
                                       threads, err, sizeof err) == FIN_EINVAL);
    }
    segs.back() = keep;
    return 0;
}

int main() {
    for (uint32_t window : {1u, 7u, 64u, 1000u})
        for (int threads : {1, 7})
            if (run(window, threads)) return 1;
    printf("ok\n");
    return 0;
}
