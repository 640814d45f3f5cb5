// fin_rows_assign (finito_amd/csrc/fin_assign_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program: no Python,
// no device, no HIP.  From the repository root:
//   g++ -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=c++17 -fopenmp -o /tmp/asan_assign tools/asan_assign.cpp \
//       finito_amd/csrc/fin_assign_host.cpp finito_amd/csrc/fin_records_host.cpp
//   /tmp/asan_assign
// Rows of 0 .. 8 colours, a zero row, a full row and the last bit of the last word, at 1, 5, 64, 65, 130 and 4096 colours, with dyadic weights (every sum exact,
// so a count made here in any order is the expectation), colour 1 weighing nothing; output buffers of exactly the size the header asks for, with one thread
// and with three, each output also left out in turn; n_rows = 0; every refusal.  It prints "ok" and exits 0 when the calls gave what they must and the
// sanitizers reported nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../include/finito_amd.h"

#define MUST(x) do { if (!(x)) { fprintf(stderr, "failed: %s (line %d, n_colors = %u, threads = %d)\n", #x, __LINE__, n_colors, threads); return 1; } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd(uint32_t n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state % n); }

static int run(uint32_t n_colors, int threads) {
    const uint32_t W = (n_colors + 63u) / 64u;
    const uint64_t n = 257;
    std::vector<double> x(n_colors), thr(n_colors);
    for (uint32_t c = 0; c < n_colors; c++) { x[c] = (double)(1 + rnd(7)) / (double)(1u << rnd(6)); thr[c] = (double)rnd(9) / 8.0; }
    if (n_colors > 1) x[1] = 0.0;
    std::vector<uint64_t> rows(n * W, 0);
    for (uint64_t r = 3; r < n; r++)
        for (uint32_t q = rnd(9); q > 0; q--) { const uint32_t c = rnd(n_colors); rows[r * W + c / 64] |= 1ull << (c & 63); }
    for (uint32_t c = 0; c < n_colors; c++) rows[1 * W + c / 64] |= 1ull << (c & 63);   // row 0 stays empty, row 1 is full, row 2 the last colour alone
    rows[2 * W + (n_colors - 1) / 64] |= 1ull << ((n_colors - 1) & 63);
    // the expectation, counted here
    std::vector<uint64_t> want_rows(n * W, 0), want_a(n_colors, 0), want_s(n_colors, 0);
    std::vector<fin_read_assign> want_h(n);
    uint64_t want_c[4] = {n, 0, 0, 0};
    for (uint64_t r = 0; r < n; r++) {
        double d = 0.0, bx = -1.0;
        uint32_t best = FIN_NO_COLOR, na = 0, last = 0;
        bool ne = false;
        for (uint32_t c = 0; c < n_colors; c++)
            if ((rows[r * W + c / 64] >> (c & 63)) & 1) { d += x[c]; ne = true; if (x[c] > bx) { bx = x[c]; best = c; } }
        for (uint32_t c = 0; c < n_colors; c++)
            if (((rows[r * W + c / 64] >> (c & 63)) & 1) && x[c] > 0.0 && d > 0.0 && x[c] >= thr[c] * d) { want_rows[r * W + c / 64] |= 1ull << (c & 63); want_a[c]++; na++; last = c; }
        if (na == 1) want_s[last]++;
        if (!ne) want_c[1]++; else if (na == 0) want_c[2]++;
        if (na >= 2) want_c[3]++;
        want_h[r].n_assigned = na; want_h[r].best = d > 0.0 ? best : FIN_NO_COLOR;
    }
    for (int leave_out = -1; leave_out < 5; leave_out++) {
        std::vector<uint64_t> out(n * W, ~0ull), a(n_colors, ~0ull), s(n_colors, ~0ull), cnt(4, ~0ull);
        std::vector<fin_read_assign> h(n);
        MUST(fin_rows_assign(rows.data(), n, n_colors, x.data(), thr.data(), leave_out == 0 ? nullptr : out.data(), leave_out == 1 ? nullptr : h.data(),
                             leave_out == 2 ? nullptr : a.data(), leave_out == 3 ? nullptr : s.data(), leave_out == 4 ? nullptr : cnt.data(), threads) == FIN_OK);
        if (leave_out != 0) MUST(out == want_rows);
        if (leave_out != 1) for (uint64_t r = 0; r < n; r++) MUST(h[r].n_assigned == want_h[r].n_assigned && h[r].best == want_h[r].best);
        if (leave_out != 2) MUST(a == want_a);
        if (leave_out != 3) MUST(s == want_s);
        if (leave_out != 4) for (int q = 0; q < 4; q++) MUST(cnt[q] == want_c[q]);
    }
    uint64_t cnt[4] = {1, 1, 1, 1};
    MUST(fin_rows_assign(nullptr, 0, n_colors, x.data(), thr.data(), nullptr, nullptr, nullptr, nullptr, cnt, threads) == FIN_OK);
    MUST(cnt[0] == 0 && cnt[1] == 0 && cnt[2] == 0 && cnt[3] == 0);
    // the refusals
    const double bad_w[] = {-1.0, std::nan(""), std::numeric_limits<double>::infinity()}, bad_t[] = {-0.5, 1.5, std::nan("")};
    for (double v : bad_w) {
        std::vector<double> y = x; y[n_colors - 1] = v;
        MUST(fin_rows_assign(rows.data(), n, n_colors, y.data(), thr.data(), nullptr, nullptr, nullptr, nullptr, cnt, threads) == FIN_EINVAL);
    }
    for (double v : bad_t) {
        std::vector<double> t = thr; t[0] = v;
        MUST(fin_rows_assign(rows.data(), n, n_colors, x.data(), t.data(), nullptr, nullptr, nullptr, nullptr, cnt, threads) == FIN_EINVAL);
    }
    if (n_colors & 63u) {
        std::vector<uint64_t> stray = rows;
        stray[(n - 1) * W + (W - 1)] |= 1ull << (n_colors & 63u);
        MUST(fin_rows_assign(stray.data(), n, n_colors, x.data(), thr.data(), nullptr, nullptr, nullptr, nullptr, cnt, threads) == FIN_EINVAL);
    }
    MUST(fin_rows_assign(rows.data(), n, 0, x.data(), thr.data(), nullptr, nullptr, nullptr, nullptr, cnt, threads) == FIN_ELIMIT);
    MUST(fin_rows_assign(rows.data(), n, FIN_MAX_COLORS + 1, x.data(), thr.data(), nullptr, nullptr, nullptr, nullptr, cnt, threads) == FIN_ELIMIT);
    MUST(fin_rows_assign(nullptr, n, n_colors, x.data(), thr.data(), nullptr, nullptr, nullptr, nullptr, cnt, threads) == FIN_EINVAL);
    return 0;
}

int main() {
    for (uint32_t n_colors : {1u, 5u, 64u, 65u, 130u, 4096u})
        for (int threads : {1, 3})
            if (run(n_colors, threads)) return 1;
    printf("ok\n");
    return 0;
}
