// fin_unitig_color_coverage (finito_amd/csrc/fin_colcov_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program:
// no Python, no device, no HIP.  From the repository root:
//   g++ -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=c++17 -fopenmp -o /tmp/asan_colcov tools/asan_colcov.cpp \
//       finito_amd/csrc/fin_colcov_host.cpp finito_amd/csrc/fin_records_host.cpp
//   /tmp/asan_colcov
// Rows of 0 .. 8 colours, an empty row, a full row and the last bit of the last word alone, at 1, 5, 64, 65, 130 and 4096 colours and 0, 1 and 257 unitigs, values
// up to 2^40 + 3; input and output buffers of exactly the size the header asks for, with one thread and with three, covered, stats and uncolored each left out
// in turn; every refusal.  The expectation is counted here colour by colour.  It prints "ok" and exits 0 when the calls gave what they must and the sanitizers
// reported nothing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/finito_amd.h"

#define MUST(x) do { if (!(x)) { fprintf(stderr, "failed: %s (line %d, n_colors = %u, n = %llu, threads = %d)\n", #x, __LINE__, n_colors, (unsigned long long)n, threads); return 1; } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd64() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static uint32_t rnd(uint32_t n) { return (uint32_t)(rnd64() % n); }

static int run(uint32_t n_colors, uint64_t n, int threads) {
    const uint32_t W = (n_colors + 63u) / 64u;
    std::vector<uint64_t> bits(n * W, 0), nk(n), cov(n);
    std::vector<fin_depth_stat> st(n);
    for (uint64_t u = 0; u < n; u++) {
        nk[u] = rnd64() % ((1ull << 40) + 4); cov[u] = rnd64() % (nk[u] + 1);
        st[u].sum = rnd64() % ((1ull << 40) + 4); st[u].max = rnd(1000); st[u].n_at_least = rnd(0xFFFFFFFFu);
        if (u >= 3) for (uint32_t q = rnd(9); q > 0; q--) { const uint32_t c = rnd(n_colors); bits[u * W + c / 64] |= 1ull << (c & 63); }
    }
    if (n > 1) for (uint32_t c = 0; c < n_colors; c++) bits[1 * W + c / 64] |= 1ull << (c & 63);   // unitig 0 stays empty, 1 is full, 2 has the last colour alone
    if (n > 2) bits[2 * W + (n_colors - 1) / 64] |= 1ull << ((n_colors - 1) & 63);
    for (int leave_out = -1; leave_out < 3; leave_out++) {
        const uint64_t* p_cov = leave_out == 0 ? nullptr : cov.data();
        const fin_depth_stat* p_st = leave_out == 1 ? nullptr : st.data();
        std::vector<fin_color_coverage> want(n_colors + 1), got(n_colors);
        memset(want.data(), 0, want.size() * sizeof(fin_color_coverage));
        memset(got.data(), 0xFF, got.size() * sizeof(fin_color_coverage));
        for (uint64_t u = 0; u < n; u++) {
            uint32_t pc = 0;
            for (uint32_t w = 0; w < W; w++) pc += (uint32_t)__builtin_popcountll(bits[u * W + w]);
            const uint64_t v[4] = {nk[u], p_cov ? cov[u] : 0, p_st ? st[u].sum : 0, p_st ? st[u].n_at_least : 0};
            for (uint32_t c = 0; c <= n_colors; c++) {
                const bool has = c < n_colors ? (bits[u * W + c / 64] >> (c & 63)) & 1 : pc == 0;
                if (!has) continue;
                fin_color_coverage& e = want[c];
                e.kmers += v[0]; e.covered += v[1]; e.depth_sum += v[2]; e.solid += v[3];
                if (c < n_colors && pc == 1) { e.kmers_only += v[0]; e.covered_only += v[1]; e.depth_sum_only += v[2]; e.solid_only += v[3]; }
            }
        }
        fin_color_coverage none;
        memset(&none, 0xFF, sizeof none);
        MUST(fin_unitig_color_coverage(n ? bits.data() : nullptr, n, n_colors, n ? nk.data() : nullptr, n ? p_cov : nullptr, n ? p_st : nullptr, got.data(),
                                       leave_out == 2 ? nullptr : &none, threads) == FIN_OK);
        MUST(memcmp(got.data(), want.data(), got.size() * sizeof(fin_color_coverage)) == 0);
        if (leave_out != 2) MUST(memcmp(&none, &want[n_colors], sizeof none) == 0);
    }
    // the refusals
    std::vector<fin_color_coverage> got(n_colors);
    if ((n_colors & 63u) && n) {
        std::vector<uint64_t> stray = bits;
        stray[(n - 1) * W + (W - 1)] |= 1ull << (n_colors & 63u);
        MUST(fin_unitig_color_coverage(stray.data(), n, n_colors, nk.data(), cov.data(), st.data(), got.data(), nullptr, threads) == FIN_EINVAL);
    }
    MUST(fin_unitig_color_coverage(bits.data(), n, 0, nk.data(), cov.data(), st.data(), got.data(), nullptr, threads) == FIN_ELIMIT);
    MUST(fin_unitig_color_coverage(bits.data(), n, FIN_MAX_COLORS + 1, nk.data(), cov.data(), st.data(), got.data(), nullptr, threads) == FIN_ELIMIT);
    MUST(fin_unitig_color_coverage(bits.data(), n, n_colors, nk.data(), cov.data(), st.data(), nullptr, nullptr, threads) == FIN_EINVAL);
    if (n) MUST(fin_unitig_color_coverage(nullptr, n, n_colors, nk.data(), cov.data(), st.data(), got.data(), nullptr, threads) == FIN_EINVAL);
    if (n) MUST(fin_unitig_color_coverage(bits.data(), n, n_colors, nullptr, cov.data(), st.data(), got.data(), nullptr, threads) == FIN_EINVAL);
    return 0;
}

int main() {
    for (uint32_t n_colors : {1u, 5u, 64u, 65u, 130u, 4096u})
        for (uint64_t n : {0ull, 1ull, 257ull})
            for (int threads : {1, 3})
                if (run(n_colors, n, threads)) return 1;
    printf("ok\n");
    return 0;
}
