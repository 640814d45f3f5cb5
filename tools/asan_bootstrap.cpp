// The bootstrap's host twins (fin_classes_resample, fin_classes_bootstrap) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone
// program: no Python, no device.  From finito_amd/csrc, in a built tree:
//   g++ -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=c++17 -fopenmp -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -c -o /tmp/capi_san.o fin_capi.cpp
//   g++ -O1 -g -fsanitize=address,undefined -std=c++17 -fopenmp -o /tmp/asan_bootstrap ../../tools/asan_bootstrap.cpp /tmp/capi_san.o \
//       $(ls *.o | grep -v fin_capi.o) -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib && /tmp/asan_bootstrap
// It prints "ok" and exits 0 when the calls gave what they must and the sanitizers reported nothing.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/finito_amd.h"

#define MUST(x) do { if (!(x)) { fprintf(stderr, "failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

int main() {
    for (uint32_t n_colors : {1u, 5u, 64u, 65u, 130u, 4096u}) {
        const uint32_t W = (n_colors + 63u) / 64u;
        const uint64_t reads_of[] = {1, 2, 3, 4, 5, 4095, 4096, 4097, 8193, 1u << 20};
        const uint64_t C = n_colors == 1 ? 1 : 10;
        std::vector<uint64_t> rows(C * W, 0), reads(C), counts(C), perm_rows(C * W), perm_reads(C), perm_counts(C);
        for (uint64_t j = 0; j < C; j++) {   // distinct non-empty rows: colour j % n_colors, and for the later classes colour (j + 1) % n_colors as well
            const uint32_t a = (uint32_t)(j % n_colors), b = (uint32_t)((j + 1) % n_colors);
            rows[j * W + a / 64] |= 1ull << (a & 63);
            if (j >= n_colors) rows[j * W + b / 64] |= 1ull << (b & 63);
            reads[j] = reads_of[j];
        }
        for (int threads : {1, 3}) {
            MUST(fin_classes_resample(rows.data(), reads.data(), C, n_colors, 0xFFFFFFFFFFFFFFFFull, 4095, counts.data(), threads) == FIN_OK);
            for (uint64_t j = 0; j < C; j++) {   // the order does not matter
                const uint64_t k = C - 1 - j;
                for (uint32_t w = 0; w < W; w++) perm_rows[k * W + w] = rows[j * W + w];
                perm_reads[k] = reads[j];
            }
            MUST(fin_classes_resample(perm_rows.data(), perm_reads.data(), C, n_colors, 0xFFFFFFFFFFFFFFFFull, 4095, perm_counts.data(), threads) == FIN_OK);
            for (uint64_t j = 0; j < C; j++) MUST(perm_counts[C - 1 - j] == counts[j] && counts[j] <= 13 * reads[j]);
        }
        MUST(fin_classes_resample(rows.data(), reads.data(), C, n_colors, 0, 4096, counts.data(), 1) == FIN_ELIMIT);
        const uint32_t n_boot = 5;
        std::vector<double> alpha(n_colors), boot((size_t)n_boot * n_colors), lens(n_colors);
        for (uint32_t c = 0; c < n_colors; c++) lens[c] = 1.0 + c % 7;
        std::vector<uint64_t> boot_reads(n_boot);
        std::vector<uint32_t> boot_iters(n_boot);
        std::vector<uint8_t> boot_conv(n_boot);
        fin_abundance_info info;
        MUST(fin_classes_bootstrap(rows.data(), reads.data(), C, n_colors, lens.data(), 25, 1e-6, n_boot, 77, alpha.data(), &info, boot.data(), boot_reads.data(), boot_iters.data(),
                                   boot_conv.data(), 3) == FIN_OK);
        for (uint32_t b = 0; b < n_boot; b++) {
            double sum = 0.0;
            for (uint32_t c = 0; c < n_colors; c++) sum += boot[(size_t)b * n_colors + c];
            if (boot_reads[b] == 0) MUST(boot_iters[b] == 0 && sum == 0.0);   // (one class of one read: an empty replicate)
            else MUST(boot_iters[b] >= 1 && boot_iters[b] <= 25 && sum > 0.999999 * boot_reads[b] && sum < 1.000001 * boot_reads[b]);
        }
        MUST(fin_classes_bootstrap(rows.data(), reads.data(), C, n_colors, nullptr, 25, 1e-6, 0, 77, alpha.data(), &info, boot.data(), boot_reads.data(), boot_iters.data(),
                                   boot_conv.data(), 1) == FIN_EINVAL);
        MUST(fin_classes_bootstrap(rows.data(), reads.data(), C, n_colors, nullptr, 25, 1e-6, 4097, 77, alpha.data(), &info, boot.data(), boot_reads.data(), boot_iters.data(),
                                   boot_conv.data(), 1) == FIN_ELIMIT);
        // N = 1: some replicates are empty; no classes: all are
        const uint64_t one_read = 1;
        std::vector<double> boot16((size_t)16 * n_colors);
        std::vector<uint64_t> r16(16); std::vector<uint32_t> i16(16); std::vector<uint8_t> c16(16);
        MUST(fin_classes_bootstrap(rows.data(), &one_read, 1, n_colors, nullptr, 10, 1e-6, 16, 2650, alpha.data(), nullptr, boot16.data(), r16.data(), i16.data(), c16.data(), 2) == FIN_OK);
        for (uint32_t b = 0; b < 16; b++) MUST((r16[b] == 0) == (i16[b] == 0) && c16[b] == 1);
        MUST(fin_classes_bootstrap(nullptr, nullptr, 0, n_colors, nullptr, 10, 1e-6, 16, 1, alpha.data(), &info, boot16.data(), r16.data(), i16.data(), c16.data(), 2) == FIN_OK);
        for (uint32_t b = 0; b < 16; b++) MUST(r16[b] == 0 && i16[b] == 0 && c16[b] == 1);
    }
    char err[256];
    MUST(fin_bootstrap_check((1ull << 26) + 1, 4096, err, sizeof err) == FIN_ELIMIT && fin_bootstrap_check(1ull << 26, 4096, err, sizeof err) == FIN_OK);
    MUST(fin_bootstrap_check(1, 4096, err, 4) == FIN_OK && fin_bootstrap_check(~0ull, 4096, err, 4) == FIN_ELIMIT);   // a short message buffer
    puts("ok");
    return 0;
}
