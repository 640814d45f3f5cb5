// fin_unitig_color_shared (finito_amd/csrc/fin_colsim_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program:
// no Python, no device, no HIP.  From the repository root:
//   g++ -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=c++17 -fopenmp -o /tmp/asan_colsim tools/asan_colsim.cpp \
//       finito_amd/csrc/fin_colsim_host.cpp finito_amd/csrc/fin_records_host.cpp
//   /tmp/asan_colsim
// Rows of 0 .. 8 colours, an empty row, a full row and the last bit of the last word alone, at 1, 5, 64, 65, 130 and 4096 colours and 0, 1 and 257 unitigs, weights
// up to 2^40 + 3 and (at 5 colours) up to 2^64 - 1, so that sums wrap; input and output buffers of exactly the size the header asks for, with one thread and with
// three; every refusal.  The expectation is counted here pair by pair.  It prints "ok" and exits 0 when the calls gave what they must and the sanitizers
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
    std::vector<uint64_t> bits(n * W, 0), v(n);
    for (uint64_t u = 0; u < n; u++) {
        v[u] = n_colors == 5 ? rnd64() : rnd64() % ((1ull << 40) + 4);
        if (u >= 3) for (uint32_t q = rnd(9); q > 0; q--) { const uint32_t c = rnd(n_colors); bits[u * W + c / 64] |= 1ull << (c & 63); }
    }
    if (n > 1) for (uint32_t c = 0; c < n_colors; c++) bits[1 * W + c / 64] |= 1ull << (c & 63);   // unitig 0 stays empty, 1 is full, 2 has the last colour alone
    if (n > 2) bits[2 * W + (n_colors - 1) / 64] |= 1ull << ((n_colors - 1) & 63);
    const size_t cells = (size_t)n_colors * n_colors;
    std::vector<uint64_t> want(cells, 0), got(cells, ~0ull);
    std::vector<uint32_t> cs;
    for (uint64_t u = 0; u < n; u++) {
        cs.clear();
        for (uint32_t c = 0; c < n_colors; c++) if ((bits[u * W + c / 64] >> (c & 63)) & 1) cs.push_back(c);
        for (uint32_t a : cs) for (uint32_t b : cs) want[(size_t)a * n_colors + b] += v[u];
    }
    MUST(fin_unitig_color_shared(n ? bits.data() : nullptr, n, n_colors, n ? v.data() : nullptr, got.data(), threads) == FIN_OK);
    MUST(memcmp(got.data(), want.data(), cells * 8) == 0);
    // the refusals
    if ((n_colors & 63u) && n) {
        std::vector<uint64_t> stray = bits;
        stray[(n - 1) * W + (W - 1)] |= 1ull << (n_colors & 63u);
        MUST(fin_unitig_color_shared(stray.data(), n, n_colors, v.data(), got.data(), threads) == FIN_EINVAL);
    }
    MUST(fin_unitig_color_shared(bits.data(), n, 0, v.data(), got.data(), threads) == FIN_ELIMIT);
    MUST(fin_unitig_color_shared(bits.data(), n, FIN_MAX_COLORS + 1, v.data(), got.data(), threads) == FIN_ELIMIT);
    MUST(fin_unitig_color_shared(bits.data(), n, n_colors, v.data(), nullptr, threads) == FIN_EINVAL);
    if (n) MUST(fin_unitig_color_shared(nullptr, n, n_colors, v.data(), got.data(), threads) == FIN_EINVAL);
    if (n) MUST(fin_unitig_color_shared(bits.data(), n, n_colors, nullptr, got.data(), threads) == FIN_EINVAL);
    MUST(memcmp(got.data(), want.data(), cells * 8) == 0);   // (a refusal writes nothing)
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
