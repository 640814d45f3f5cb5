// fin_colorsets_host.cpp -- the host twin of fin_colorsets.hip (include/finito_amd.h: fin_unitig_color_sets, fin_color_sets_expand): the
// definition and the CANONICAL form of the deduplicated colour sets, no device, no HIP header.  Plain C++ with OpenMP.
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/finito_amd.h"

int fin_unitig_color_sets(const uint64_t* bits, uint64_t n_unitigs, uint32_t n_colors, uint32_t* set_of_out, uint64_t* sets_out, uint64_t cap_sets, uint64_t* n_sets,
                          int n_threads) {
    if (n_sets) *n_sets = 0;
    if (n_colors == 0 || n_colors > FIN_MAX_COLORS || n_unitigs >= 0x80000000ull) return FIN_ELIMIT;
    if ((n_unitigs && !bits) || !n_sets) return FIN_EINVAL;
    const uint32_t W = (n_colors + 63u) / 64u;
    const uint64_t stray = (n_colors & 63u) ? ~0ull << (n_colors & 63u) : 0ull;
    for (uint64_t u = 0; u < n_unitigs; u++) if (bits[u * W + (W - 1)] & stray) return FIN_EINVAL;
    const int T = std::max(1, n_threads > 0 ? n_threads : fin_host_threads());
    auto row = [&](uint32_t u) { return bits + (size_t)u * W; };
    auto less = [&](uint32_t a, uint32_t b) {   // ascending by word 0, then word 1, ...: np.unique(axis=0)'s order
        const uint64_t *ra = row(a), *rb = row(b);
        for (uint32_t w = 0; w < W; w++) if (ra[w] != rb[w]) return ra[w] < rb[w];
        return false;
    };
    auto empty = [&](uint32_t u) { const uint64_t* r = row(u); for (uint32_t w = 0; w < W; w++) if (r[w]) return false; return true; };
    std::vector<uint32_t> order;            // the non-empty rows' unitigs, sorted by row
    order.reserve((size_t)n_unitigs);
    for (uint64_t u = 0; u < n_unitigs; u++) if (!empty((uint32_t)u)) order.push_back((uint32_t)u);
    // T runs sorted side by side, then merged pairwise, a round at a time: the result is the sorted list whatever T is
    const size_t n_ne = order.size();
    const size_t runs = (size_t)std::max(1, std::min<int>(T, (int)(n_ne / 4096) + 1));
    auto cut = [&](size_t r) { return n_ne * r / runs; };
#pragma omp parallel for schedule(static) num_threads(T)
    for (int64_t r = 0; r < (int64_t)runs; r++) std::sort(order.begin() + cut((size_t)r), order.begin() + cut((size_t)r + 1), less);
    for (size_t width = 1; width < runs; width *= 2) {
#pragma omp parallel for schedule(static) num_threads(T)
        for (int64_t r = 0; r < (int64_t)runs; r += 2 * (int64_t)width)
            if ((size_t)r + width < runs)
                std::inplace_merge(order.begin() + cut((size_t)r), order.begin() + cut((size_t)r + width), order.begin() + cut(std::min(runs, (size_t)r + 2 * width)), less);
    }
    std::vector<uint32_t> reps;             // the first unitig of every distinct row, ascending by row
    for (size_t i = 0; i < order.size(); i++) if (i == 0 || less(order[i - 1], order[i])) reps.push_back(order[i]);
    *n_sets = reps.size();
    if (cap_sets < reps.size() + 1) return FIN_ELIMIT;
    if (sets_out) {
        memset(sets_out, 0, (size_t)W * 8);
        for (size_t s = 0; s < reps.size(); s++) memcpy(sets_out + (s + 1) * W, row(reps[s]), (size_t)W * 8);
    }
    if (set_of_out) {
        const int64_t n = (int64_t)n_unitigs;
#pragma omp parallel for schedule(static) num_threads(T)
        for (int64_t u = 0; u < n; u++) {
            if (empty((uint32_t)u)) { set_of_out[u] = 0; continue; }
            // the first representative whose row is not below this one is this row's
            const size_t s = (size_t)(std::lower_bound(reps.begin(), reps.end(), (uint32_t)u, less) - reps.begin());
            set_of_out[u] = (uint32_t)s + 1u;
        }
    }
    return FIN_OK;
}

int fin_color_sets_expand(const uint32_t* set_of, const uint64_t* sets, uint64_t n_unitigs, uint64_t n_sets, uint32_t n_colors, uint64_t* bits_out, int n_threads) {
    if (n_colors == 0 || n_colors > FIN_MAX_COLORS || n_sets > 0xFFFFFFFEull) return FIN_ELIMIT;
    if (!sets || (n_unitigs && (!set_of || !bits_out))) return FIN_EINVAL;
    const uint32_t W = (n_colors + 63u) / 64u;
    const uint64_t stray = (n_colors & 63u) ? ~0ull << (n_colors & 63u) : 0ull;
    for (uint32_t w = 0; w < W; w++) if (sets[w]) return FIN_EINVAL;
    for (uint64_t s = 0; s <= n_sets; s++) if (sets[s * W + (W - 1)] & stray) return FIN_EINVAL;
    for (uint64_t u = 0; u < n_unitigs; u++) if (set_of[u] > n_sets) return FIN_EINVAL;
    const int T = n_threads > 0 ? n_threads : fin_host_threads();
    const int64_t n = (int64_t)n_unitigs;
#pragma omp parallel for schedule(static) num_threads(T)
    for (int64_t u = 0; u < n; u++) memcpy(bits_out + (size_t)u * W, sets + (size_t)set_of[u] * W, (size_t)W * 8);
    return FIN_OK;
}
