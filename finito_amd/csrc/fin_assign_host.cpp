// fin_assign_host.cpp -- the host twin of fin_assign.hip (include/finito_amd.h: fin_rows_assign): the definition in the stated order, no device,
// no HIP header.  Plain C++ with OpenMP: tools/asan_assign.cpp compiles this file beside fin_records_host.cpp (fin_host_threads).
#include <math.h>
#include <string.h>

#include <vector>

#include "../../include/finito_amd.h"

// the refusals fin_assign_create and fin_assign_set share with the twin: the first colour whose weight is negative, NaN or infinite (*what = 0) or whose
// threshold is outside [0, 1] or NaN (*what = 1); n_colors: none
extern "C" uint32_t fin_assign_first_bad(const double* weights, const double* thresholds, uint32_t n_colors, int* what) {
    for (uint32_t c = 0; c < n_colors; c++) {
        if (!(weights[c] >= 0.0) || !std::isfinite(weights[c])) { *what = 0; return c; }
        if (!(thresholds[c] >= 0.0 && thresholds[c] <= 1.0)) { *what = 1; return c; }
    }
    return n_colors;
}

int fin_rows_assign(const uint64_t* rows, uint64_t n_rows, uint32_t n_colors, const double* weights, const double* thresholds, uint64_t* out_rows, fin_read_assign* heads,
                    uint64_t* assigned, uint64_t* sole, uint64_t counters[4], int n_threads) {
    if (n_colors == 0 || n_colors > FIN_MAX_COLORS) return FIN_ELIMIT;
    if ((n_rows && !rows) || !weights || !thresholds) return FIN_EINVAL;
    int what = 0;
    if (fin_assign_first_bad(weights, thresholds, n_colors, &what) != n_colors) return FIN_EINVAL;
    const uint32_t W = (n_colors + 63u) / 64u;
    uint32_t wp2 = 1;
    while (wp2 < W) wp2 <<= 1;
    const uint64_t stray = (n_colors & 63u) ? ~0ull << (n_colors & 63u) : 0ull;
    for (uint64_t r = 0; r < n_rows; r++) if (rows[r * W + (W - 1)] & stray) return FIN_EINVAL;
    const int T = n_threads > 0 ? n_threads : fin_host_threads();
    const int64_t n = (int64_t)n_rows;
    // every count is an integer: a thread counts its rows by itself, the threads' counts are added up -- whatever the number of threads
    std::vector<uint64_t> part_a((size_t)T * n_colors, 0), part_s((size_t)T * n_colors, 0), part_c((size_t)T * 4, 0);
#pragma omp parallel num_threads(T)
    {
        std::vector<double> s(wp2);
        std::vector<uint64_t> a(W);
#pragma omp for schedule(static)
        for (int t = 0; t < T; t++) {
            uint64_t* const pa = part_a.data() + (size_t)t * n_colors;
            uint64_t* const ps = part_s.data() + (size_t)t * n_colors;
            uint64_t* const pc = part_c.data() + (size_t)t * 4;
            for (int64_t r = n * t / T; r < n * (t + 1) / T; r++) {
                const uint64_t* row = rows + (size_t)r * W;
                bool ne = false;
                double bx = -1.0;
                uint32_t best = FIN_NO_COLOR;
                for (uint32_t w = 0; w < wp2; w++) {
                    double sw = 0.0;
                    if (w < W)
                        for (uint64_t m = row[w]; m; m &= m - 1) {
                            const uint32_t c = 64u * w + (uint32_t)__builtin_ctzll(m);
                            sw += weights[c];
                            if (weights[c] > bx) { bx = weights[c]; best = c; }
                            ne = true;
                        }
                    s[w] = sw;
                }
                for (uint32_t h = wp2 >> 1; h >= 1u; h >>= 1) for (uint32_t i = 0; i < h; i++) s[i] = s[i] + s[i + h];
                const double d = s[0];
                uint32_t na = 0, last = 0;
                for (uint32_t w = 0; w < W; w++) {
                    uint64_t aw = 0;
                    for (uint64_t m = row[w]; m; m &= m - 1) {
                        const uint32_t b = (uint32_t)__builtin_ctzll(m), c = 64u * w + b;
                        const double x = weights[c];
                        if (x > 0.0 && d > 0.0 && x >= thresholds[c] * d) { aw |= 1ull << b; last = c; na++; pa[c]++; }
                    }
                    a[w] = aw;
                }
                if (na == 1u) ps[last]++;
                pc[0]++;
                if (!ne) pc[1]++;
                else if (na == 0u) pc[2]++;
                if (na >= 2u) pc[3]++;
                if (out_rows) memcpy(out_rows + (size_t)r * W, a.data(), (size_t)W * 8);
                if (heads) { heads[r].n_assigned = na; heads[r].best = d > 0.0 ? best : FIN_NO_COLOR; }
            }
        }
    }
    for (uint32_t c = 0; c < n_colors; c++) {
        uint64_t va = 0, vs = 0;
        for (int t = 0; t < T; t++) { va += part_a[(size_t)t * n_colors + c]; vs += part_s[(size_t)t * n_colors + c]; }
        if (assigned) assigned[c] = va;
        if (sole) sole[c] = vs;
    }
    if (counters)
        for (int q = 0; q < 4; q++) {
            uint64_t v = 0;
            for (int t = 0; t < T; t++) v += part_c[(size_t)t * 4 + q];
            counters[q] = v;
        }
    return FIN_OK;
}
