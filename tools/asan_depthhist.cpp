// fin_depth_positions_histogram and fin_unitig_color_depth_histogram (finito_amd/csrc/fin_depthhist_host.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer, as a stand-alone program: no Python, no device, no HIP.  From the repository root:
//   g++ -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=c++17 -fopenmp -o /tmp/asan_depthhist tools/asan_depthhist.cpp \
//       finito_amd/csrc/fin_depthhist_host.cpp finito_amd/csrc/fin_records_host.cpp finito_amd/csrc/fin_taxa_host.cpp
//   /tmp/asan_depthhist
// Hand-made unitigs -- one shorter than k, one of exactly k, the last one shorter than k again --, depths on every bin edge and 2^32 - 1, non-zero depths over the
// last k - 1 positions of every unitig, n_bins 1, 2, 65 and 1024, bin widths 1, 3 and 2^30, 1, 5, 65 and 4096 colours, one thread and seven; input and output
// buffers of exactly the size the header asks for; every refusal.  The expectation is counted here position by position.  It prints "ok" and exits 0 when the calls
// gave what they must and the sanitizers reported nothing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/finito_amd.h"

#define MUST(x) do { if (!(x)) { fprintf(stderr, "failed: %s (line %d, n_colors = %u, n_bins = %u, bin_width = %u, threads = %d)\n", #x, __LINE__, n_colors, n_bins, bw, threads); return 1; } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd64() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static uint32_t rnd(uint32_t n) { return (uint32_t)(rnd64() % n); }

static int run(uint32_t n_colors, uint32_t n_bins, uint32_t bw, int threads) {
    const int k = 5;
    const uint32_t W = (n_colors + 63u) / 64u;
    const std::vector<int64_t> lens = {4, 5, 6, 23, 9, 40, 5, 17, 4};   // unitig 0 and the last are shorter than k, 1 and 6 hold one k-mer
    const uint64_t n = lens.size();
    std::vector<int64_t> ends(n);
    int64_t total = 0;
    for (uint64_t u = 0; u < n; u++) { total += lens[u]; ends[u] = total; }
    const uint64_t top = (uint64_t)(n_bins - 1u) * bw;
    const uint64_t edges[] = {0, bw - 1ull, bw, top ? top - 1 : 0, top, top + 1, 0xFFFFFFFFull};
    std::vector<uint32_t> depth((size_t)total);
    for (int64_t g = 0; g < total; g++) {
        const uint64_t e = edges[rnd(7)];
        depth[(size_t)g] = rnd(3) == 0 && e <= 0xFFFFFFFFull ? (uint32_t)e : rnd(2u * n_bins) * (rnd(2) ? bw : 1u);
    }
    std::vector<uint64_t> bits(n * W, 0);
    for (uint64_t u = 3; u < n; u++) for (uint32_t q = rnd(4); q > 0; q--) { const uint32_t c = rnd(n_colors); bits[u * W + c / 64] |= 1ull << (c & 63); }
    for (uint32_t c = 0; c < n_colors; c++) bits[1 * W + c / 64] |= 1ull << (c & 63);   // unitig 0 stays empty, 1 is full, 2 has the last colour alone
    bits[2 * W + (n_colors - 1) / 64] |= 1ull << ((n_colors - 1) & 63);
    const size_t cells = (size_t)n_colors * 2u * n_bins;
    std::vector<uint64_t> want(cells, 0), want_none(n_bins, 0), want_hist(n_bins, 0), got(cells, ~0ull), got_none(n_bins, ~0ull), got_hist(n_bins, ~0ull);
    int64_t s = 0;
    for (uint64_t u = 0; u < n; u++) {
        uint32_t pc = 0;
        for (uint32_t w = 0; w < W; w++) pc += (uint32_t)__builtin_popcountll(bits[u * W + w]);
        for (int64_t g = s; g + k <= ends[u]; g++) {
            uint64_t b = depth[(size_t)g] / bw;
            if (b > n_bins - 1u) b = n_bins - 1u;
            want_hist[b]++;
            if (pc == 0) want_none[b]++;
            for (uint32_t c = 0; c < n_colors; c++)
                if ((bits[u * W + c / 64] >> (c & 63)) & 1) { want[((size_t)c * 2u) * n_bins + b]++; if (pc == 1) want[((size_t)c * 2u + 1u) * n_bins + b]++; }
        }
        s = ends[u];
    }
    MUST(fin_depth_positions_histogram(depth.data(), ends.data(), n, k, n_bins, bw, got_hist.data(), threads) == FIN_OK);
    MUST(memcmp(got_hist.data(), want_hist.data(), (size_t)n_bins * 8) == 0);
    MUST(fin_unitig_color_depth_histogram(depth.data(), ends.data(), n, k, bits.data(), n_colors, n_bins, bw, got.data(), got_none.data(), threads) == FIN_OK);
    MUST(memcmp(got.data(), want.data(), cells * 8) == 0 && memcmp(got_none.data(), want_none.data(), (size_t)n_bins * 8) == 0);
    MUST(fin_unitig_color_depth_histogram(depth.data(), ends.data(), n, k, bits.data(), n_colors, n_bins, bw, got.data(), nullptr, threads) == FIN_OK);   // (uncolored may be NULL)
    // no unitigs at all
    std::vector<uint64_t> zero(cells, ~0ull);
    MUST(fin_unitig_color_depth_histogram(nullptr, nullptr, 0, k, nullptr, n_colors, n_bins, bw, zero.data(), nullptr, threads) == FIN_OK);
    for (uint64_t v : zero) MUST(v == 0);
    MUST(fin_depth_positions_histogram(nullptr, nullptr, 0, k, n_bins, bw, got_hist.data(), threads) == FIN_OK);
    for (uint64_t v : got_hist) MUST(v == 0);
    // the refusals
    if (n_colors & 63u) {
        std::vector<uint64_t> stray = bits;
        stray[(n - 1) * W + (W - 1)] |= 1ull << (n_colors & 63u);
        MUST(fin_unitig_color_depth_histogram(depth.data(), ends.data(), n, k, stray.data(), n_colors, n_bins, bw, got.data(), nullptr, threads) == FIN_EINVAL);
    }
    MUST(fin_unitig_color_depth_histogram(depth.data(), ends.data(), n, k, bits.data(), 0, n_bins, bw, got.data(), nullptr, threads) == FIN_ELIMIT);
    MUST(fin_unitig_color_depth_histogram(depth.data(), ends.data(), n, k, bits.data(), FIN_MAX_COLORS + 1, n_bins, bw, got.data(), nullptr, threads) == FIN_ELIMIT);
    MUST(fin_unitig_color_depth_histogram(depth.data(), ends.data(), n, k, bits.data(), n_colors, 0, bw, got.data(), nullptr, threads) == FIN_EINVAL);
    MUST(fin_unitig_color_depth_histogram(depth.data(), ends.data(), n, k, bits.data(), n_colors, FIN_DEPTH_HIST_MAX_BINS + 1, bw, got.data(), nullptr, threads) == FIN_EINVAL);
    MUST(fin_unitig_color_depth_histogram(depth.data(), ends.data(), n, k, bits.data(), n_colors, n_bins, 0, got.data(), nullptr, threads) == FIN_EINVAL);
    MUST(fin_unitig_color_depth_histogram(depth.data(), ends.data(), n, 0, bits.data(), n_colors, n_bins, bw, got.data(), nullptr, threads) == FIN_EINVAL);
    MUST(fin_unitig_color_depth_histogram(depth.data(), ends.data(), n, k, bits.data(), n_colors, n_bins, bw, nullptr, nullptr, threads) == FIN_EINVAL);
    MUST(fin_unitig_color_depth_histogram(depth.data(), ends.data(), n, k, nullptr, n_colors, n_bins, bw, got.data(), nullptr, threads) == FIN_EINVAL);
    MUST(fin_unitig_color_depth_histogram(nullptr, ends.data(), n, k, bits.data(), n_colors, n_bins, bw, got.data(), nullptr, threads) == FIN_EINVAL);
    MUST(fin_depth_positions_histogram(depth.data(), ends.data(), n, k, n_bins, bw, nullptr, threads) == FIN_EINVAL);
    MUST(fin_depth_positions_histogram(depth.data(), nullptr, n, k, n_bins, bw, got_hist.data(), threads) == FIN_EINVAL);
    MUST(memcmp(got.data(), want.data(), cells * 8) == 0);   // (a refusal writes nothing)
    return 0;
}

int main() {
    for (uint32_t n_colors : {1u, 5u, 65u, 4096u})
        for (uint32_t n_bins : {1u, 2u, 65u, 1024u})
            for (uint32_t bw : {1u, 3u, 1u << 30})
                for (int threads : {1, 7}) {
                    if (n_colors == 4096u && n_bins == 1024u && bw != 1u) continue;   // (64 MB a table: once is enough)
                    if (run(n_colors, n_bins, bw, threads)) return 1;
                }
    printf("ok\n");
    return 0;
}
