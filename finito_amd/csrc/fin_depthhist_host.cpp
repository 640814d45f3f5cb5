// fin_depthhist_host.cpp -- the host twins of fin_depthhist.hip (include/finito_amd.h: fin_depth_positions_histogram, fin_unitig_color_depth_histogram; DESIGN.md
// 4.26): the definitions, no device, no HIP header.  Plain C++ with OpenMP: tools/asan_depthhist.cpp compiles this file beside fin_records_host.cpp
// (fin_host_threads).
#include <string.h>

#include <vector>

#include "../../include/finito_amd.h"

namespace {
bool dh_args_ok(const uint32_t* depth, const int64_t* ends, uint64_t n_unitigs, int k, uint32_t n_bins, uint32_t bin_width) {
    if (k < 1 || n_bins == 0 || n_bins > FIN_DEPTH_HIST_MAX_BINS || bin_width == 0) return false;
    if (n_unitigs && !ends) return false;
    int64_t at = 0;
    for (uint64_t u = 0; u < n_unitigs; u++) { if (ends[u] < at) return false; at = ends[u]; }
    return at == 0 || depth;
}
// h[bin] += 1 for every position of unitig u at which a k-mer begins
inline void dh_unitig(const uint32_t* depth, const int64_t* ends, uint64_t u, int k, uint32_t n_bins, uint32_t bin_width, uint64_t* h) {
    const int64_t s = u ? ends[u - 1] : 0, nk = ends[u] - s - k + 1;
    for (int64_t g = s; g < s + nk; g++) {
        const uint32_t q = depth[g] / bin_width;
        h[q < n_bins - 1u ? q : n_bins - 1u]++;
    }
}
}  // namespace

int fin_depth_positions_histogram(const uint32_t* depth, const int64_t* unitig_ends, uint64_t n_unitigs, int k, uint32_t n_bins, uint32_t bin_width, uint64_t* hist_out,
                                  int n_threads) {
    if (!hist_out || !dh_args_ok(depth, unitig_ends, n_unitigs, k, n_bins, bin_width)) return FIN_EINVAL;
    const int T = n_threads > 0 ? n_threads : fin_host_threads();
    const int64_t n = (int64_t)n_unitigs;
    // every count is an integer: a thread counts its unitigs by itself, the threads' tables are added up -- whatever the number of threads
    std::vector<uint64_t> part((size_t)T * n_bins, 0);
#pragma omp parallel for schedule(static) num_threads(T)
    for (int t = 0; t < T; t++)
        for (int64_t u = n * t / T; u < n * (t + 1) / T; u++) dh_unitig(depth, unitig_ends, (uint64_t)u, k, n_bins, bin_width, part.data() + (size_t)t * n_bins);
    for (uint32_t b = 0; b < n_bins; b++) {
        uint64_t s = 0;
        for (int t = 0; t < T; t++) s += part[(size_t)t * n_bins + b];
        hist_out[b] = s;
    }
    return FIN_OK;
}

int fin_unitig_color_depth_histogram(const uint32_t* depth, const int64_t* unitig_ends, uint64_t n_unitigs, int k, const uint64_t* bits, uint32_t n_colors, uint32_t n_bins,
                                     uint32_t bin_width, uint64_t* out, uint64_t* uncolored, int n_threads) {
    if (n_colors == 0 || n_colors > FIN_MAX_COLORS) return FIN_ELIMIT;
    if (!out || (n_unitigs && !bits) || !dh_args_ok(depth, unitig_ends, n_unitigs, k, n_bins, bin_width)) return FIN_EINVAL;
    const uint32_t W = (n_colors + 63u) / 64u;
    const uint64_t stray = (n_colors & 63u) ? ~0ull << (n_colors & 63u) : 0ull;
    for (uint64_t u = 0; u < n_unitigs; u++) if (bits[u * W + (W - 1)] & stray) return FIN_EINVAL;
    int T = n_threads > 0 ? n_threads : fin_host_threads();
    if ((uint64_t)T > n_unitigs) T = n_unitigs ? (int)n_unitigs : 1;   // (a thread without unitigs would only zero a table)
    const int64_t n = (int64_t)n_unitigs;
    const size_t cells = ((size_t)n_colors * 2u + 1u) * n_bins;   // per thread: [n_colors][2][n_bins], then the uncoloured histogram
    std::vector<std::vector<uint64_t>> part((size_t)T);   // (a thread makes its own table: first touch puts its pages beside it)
#pragma omp parallel for schedule(static) num_threads(T)
    for (int t = 0; t < T; t++) {
        part[(size_t)t].assign(cells, 0);
        std::vector<uint64_t>& tab = part[(size_t)t];
        std::vector<uint64_t> h(n_bins);
        std::vector<uint32_t> nz;   // the bins of the unitig at hand that hold anything: depth is piecewise constant, so they are few
        for (int64_t u = n * t / T; u < n * (t + 1) / T; u++) {
            const uint64_t* row = bits + (size_t)u * W;
            memset(h.data(), 0, (size_t)n_bins * 8u);
            dh_unitig(depth, unitig_ends, (uint64_t)u, k, n_bins, bin_width, h.data());
            nz.clear();
            for (uint32_t b = 0; b < n_bins; b++) if (h[b]) nz.push_back(b);
            uint32_t pc = 0;
            for (uint32_t w = 0; w < W; w++) pc += (uint32_t)__builtin_popcountll(row[w]);
            if (pc == 0) {
                uint64_t* const e = tab.data() + (size_t)n_colors * 2u * n_bins;
                for (uint32_t b : nz) e[b] += h[b];
                continue;
            }
            for (uint32_t w = 0; w < W; w++)
                for (uint64_t m = row[w]; m; m &= m - 1) {
                    uint64_t* const e = tab.data() + (size_t)(64u * w + (uint32_t)__builtin_ctzll(m)) * 2u * n_bins;
                    for (uint32_t b : nz) {
                        e[b] += h[b];
                        if (pc == 1) e[n_bins + b] += h[b];
                    }
                }
        }
    }
    std::vector<uint64_t> tot(cells);
#pragma omp parallel for schedule(static) num_threads(T)
    for (int64_t i = 0; i < (int64_t)cells; i++) {   // (the tables are added cell by cell, every thread a stretch of cells)
        uint64_t v = 0;
        for (int t = 0; t < T; t++) v += part[(size_t)t][(size_t)i];
        tot[(size_t)i] = v;
    }
    memcpy(out, tot.data(), (size_t)n_colors * 2u * n_bins * 8u);
    if (uncolored) memcpy(uncolored, tot.data() + (size_t)n_colors * 2u * n_bins, (size_t)n_bins * 8u);
    return FIN_OK;
}
