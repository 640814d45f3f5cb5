// fin_colsim_host.cpp -- the host twin of fin_colsim.hip (include/finito_amd.h: fin_unitig_color_shared): the definition, no device, no HIP
// header.  Plain C++ with OpenMP: tools/asan_colsim.cpp compiles this file beside fin_records_host.cpp (fin_host_threads).
#include <string.h>

#include <vector>

#include "../../include/finito_amd.h"

int fin_unitig_color_shared(const uint64_t* bits, uint64_t n_unitigs, uint32_t n_colors, const uint64_t* v, uint64_t* out, int n_threads) {
    if (n_colors == 0 || n_colors > FIN_MAX_COLORS) return FIN_ELIMIT;
    if ((n_unitigs && (!bits || !v)) || !out) return FIN_EINVAL;
    const uint32_t W = (n_colors + 63u) / 64u;
    const uint64_t stray = (n_colors & 63u) ? ~0ull << (n_colors & 63u) : 0ull;
    for (uint64_t u = 0; u < n_unitigs; u++) if (bits[u * W + (W - 1)] & stray) return FIN_EINVAL;
    const size_t cells = (size_t)n_colors * n_colors;
    // no more threads than there are blocks of 64 unitigs: a thread's table is n_colors^2 words
    int T = n_threads > 0 ? n_threads : fin_host_threads();
    if ((uint64_t)T > n_unitigs / 64u + 1u) T = (int)(n_unitigs / 64u + 1u);
    const int64_t n = (int64_t)n_unitigs;
    // every sum is an integer mod 2^64: a thread sums the upper triangle over its unitigs by itself, the threads' tables are added up -- whatever the number of threads
    std::vector<uint64_t> part((size_t)T * cells, 0);
#pragma omp parallel for schedule(static) num_threads(T)
    for (int t = 0; t < T; t++) {
        uint64_t* const tab = part.data() + (size_t)t * cells;
        std::vector<uint32_t> cs(n_colors);
        for (int64_t u = n * t / T; u < n * (t + 1) / T; u++) {
            const uint64_t* row = bits + (size_t)u * W;
            const uint64_t x = v[u];
            if (x == 0) continue;
            uint32_t m = 0;
            for (uint32_t w = 0; w < W; w++)
                for (uint64_t b = row[w]; b; b &= b - 1) cs[m++] = 64u * w + (uint32_t)__builtin_ctzll(b);
            for (uint32_t a = 0; a < m; a++) {
                uint64_t* const r = tab + (size_t)cs[a] * n_colors;
                for (uint32_t b = a; b < m; b++) r[cs[b]] += x;
            }
        }
    }
    for (int t = 1; t < T; t++)
        for (size_t i = 0; i < cells; i++) part[i] += part[(size_t)t * cells + i];
    // the upper triangle and its mirror, a tile of 64 x 64 at a time: both sides stay in the cache
    for (uint32_t i0 = 0; i0 < n_colors; i0 += 64u)
        for (uint32_t j0 = i0; j0 < n_colors; j0 += 64u)
            for (uint32_t i = i0; i < i0 + 64u && i < n_colors; i++)
                for (uint32_t j = j0 > i ? j0 : i; j < j0 + 64u && j < n_colors; j++) out[(size_t)j * n_colors + i] = out[(size_t)i * n_colors + j] = part[(size_t)i * n_colors + j];
    return FIN_OK;
}
