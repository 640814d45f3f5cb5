// fin_colcov_host.cpp -- the host twin of fin_colcov.hip (include/finito_amd.h: fin_unitig_color_coverage): the definition, no device, no HIP
// header.  Plain C++ with OpenMP: tools/asan_colcov.cpp compiles this file beside fin_records_host.cpp (fin_host_threads).
#include <string.h>

#include <vector>

#include "../../include/finito_amd.h"

static_assert(sizeof(fin_color_coverage) == 64, "fin_color_coverage is eight uint64");

int fin_unitig_color_coverage(const uint64_t* bits, uint64_t n_unitigs, uint32_t n_colors, const uint64_t* nk, const uint64_t* covered, const fin_depth_stat* stats,
                              fin_color_coverage* out, fin_color_coverage* uncolored, int n_threads) {
    if (n_colors == 0 || n_colors > FIN_MAX_COLORS) return FIN_ELIMIT;
    if ((n_unitigs && (!bits || !nk)) || !out) return FIN_EINVAL;
    const uint32_t W = (n_colors + 63u) / 64u;
    const uint64_t stray = (n_colors & 63u) ? ~0ull << (n_colors & 63u) : 0ull;
    for (uint64_t u = 0; u < n_unitigs; u++) if (bits[u * W + (W - 1)] & stray) return FIN_EINVAL;
    const int T = n_threads > 0 ? n_threads : fin_host_threads();
    const int64_t n = (int64_t)n_unitigs;
    // every sum is an integer: a thread sums its unitigs by itself, the threads' tables are added up -- whatever the number of threads
    std::vector<uint64_t> part((size_t)T * (n_colors + 1u) * 8u, 0);   // per thread: n_colors entries of eight, then the uncoloured one
#pragma omp parallel for schedule(static) num_threads(T)
    for (int t = 0; t < T; t++) {
        uint64_t* const tab = part.data() + (size_t)t * (n_colors + 1u) * 8u;
        for (int64_t u = n * t / T; u < n * (t + 1) / T; u++) {
            const uint64_t* row = bits + (size_t)u * W;
            const uint64_t v[4] = {nk[u], covered ? covered[u] : 0, stats ? stats[u].sum : 0, stats ? (uint64_t)stats[u].n_at_least : 0};
            uint32_t pc = 0;
            for (uint32_t w = 0; w < W; w++) pc += (uint32_t)__builtin_popcountll(row[w]);
            if (pc == 0) {
                uint64_t* const e = tab + (size_t)n_colors * 8u;
                for (int q = 0; q < 4; q++) e[2 * q] += v[q];
                continue;
            }
            for (uint32_t w = 0; w < W; w++)
                for (uint64_t m = row[w]; m; m &= m - 1) {
                    uint64_t* const e = tab + (size_t)(64u * w + (uint32_t)__builtin_ctzll(m)) * 8u;
                    for (int q = 0; q < 4; q++) {
                        e[2 * q] += v[q];
                        if (pc == 1) e[2 * q + 1] += v[q];
                    }
                }
        }
    }
    std::vector<uint64_t> tot((size_t)(n_colors + 1u) * 8u, 0);
    for (int t = 0; t < T; t++)
        for (size_t i = 0; i < tot.size(); i++) tot[i] += part[(size_t)t * tot.size() + i];
    memcpy(out, tot.data(), (size_t)n_colors * 64u);
    if (uncolored) memcpy(uncolored, tot.data() + (size_t)n_colors * 8u, 64u);
    return FIN_OK;
}
