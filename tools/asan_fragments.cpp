// fin_records_fragments and fin_effective_lengths (finito_amd/csrc/fin_fragments_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a
// stand-alone program: no Python, no device, no HIP.  From the repository root:
//   g++ -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=c++17 -fopenmp -o /tmp/asan_fragments tools/asan_fragments.cpp \
//       finito_amd/csrc/fin_fragments_host.cpp finito_amd/csrc/fin_records_host.cpp finito_amd/csrc/fin_taxa_host.cpp
//   /tmp/asan_fragments
// (fin_records_host.cpp provides fin_host_threads; its read-taxa twin calls fin_taxa_call and fin_taxa_first_bad_parent, which fin_taxa_host.cpp defines)
// 7000 hand-made fragments -- every mate a straight run on either strand of one of three unitigs, as a kind-1 record or as a searched read's pairs in the stream,
// or a kind-2 read, or a read without k-mers --, n_bins 1 and 4096, bin widths 1, 3 and 1000, one thread and seven; input and output buffers of exactly the size
// the header asks for; every refusal.  The expectation is worked out here from the geometry the mates were made with.  It prints "ok" and exits 0 when the calls
// gave what they must and the sanitizers reported nothing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/finito_amd.h"

#define MUST(x) do { if (!(x)) { fprintf(stderr, "failed: %s (line %d, n_bins = %u, bin_width = %u, threads = %d)\n", #x, __LINE__, n_bins, bw, threads); return 1; } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd64() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static uint32_t rnd(uint32_t n) { return (uint32_t)(rnd64() % n); }

struct Geo { bool placed; uint32_t u, s0, L; bool rev; };

static int run(uint32_t n_bins, uint32_t bw, int threads) {
    const int k = 5;
    const std::vector<int64_t> lens = {6000, 90, 7};
    std::vector<int64_t> ends;
    int64_t total = 0;
    for (int64_t l : lens) { total += l; ends.push_back(total); }
    const uint64_t n_frags = 7000, n_reads = 2 * n_frags;
    std::vector<fin_read_record> recs(n_reads);
    std::vector<int32_t> stream;
    std::vector<Geo> geo(n_reads);
    for (uint64_t r = 0; r < n_reads; r++) {
        fin_read_record& R = recs[r];
        memset(&R, 0, sizeof R);
        Geo& g = geo[r];
        g = Geo{false, 0, 0, 0, false};
        const uint32_t t = rnd(10);
        if (t == 0) { R.nk = 1 + rnd(9); R.meta = 2u << 16; continue; }   // kind 2
        if (t == 1) continue;                                             // a read without k-mers: kind 0, nk 0
        const uint32_t u = rnd(8) ? 0u : 1u + rnd(2), kmers = (uint32_t)lens[u] - (uint32_t)k + 1u;
        const uint32_t nk = 1u + rnd(kmers < 40u ? kmers : 40u), s0 = rnd(kmers - nk + 1u);
        const bool rev = rnd(2);
        g = Geo{nk >= 2u, u, s0, nk + (uint32_t)k - 1u, rev};               // (one slot does not tell the strand)
        R.nk = nk;
        if (rnd(2)) { R.u = u; R.off0 = s0; R.meta = (1u << 16) | (rev ? 0x100u : 0u); }
        else for (uint32_t i = 0; i < nk; i++) { stream.push_back((int32_t)u); stream.push_back((int32_t)(s0 + (rev ? nk - 1u - i : i))); }
    }
    std::vector<fin_fragment> want(n_frags), got(n_frags);
    std::vector<uint64_t> want_hist(n_bins, 0), got_hist(n_bins, ~0ull);
    uint64_t want_cnt[7] = {0, 0, 0, 0, 0, 0, 0}, got_cnt[7];
    for (uint64_t f = 0; f < n_frags; f++) {
        const Geo &a = geo[2 * f], &b = geo[2 * f + 1];
        const uint32_t bits = (a.placed && a.rev ? 0x100u : 0u) | (b.placed && b.rev ? 0x200u : 0u) | (a.placed ? 0x400u : 0u) | (b.placed ? 0x800u : 0u);
        fin_fragment w = {0xFFFFFFFFu, 0u, 0u, 0u};
        if (a.placed != b.placed) { const Geo& m = a.placed ? a : b; w = fin_fragment{m.u, m.s0, m.L, FIN_FRAG_ONE}; }
        else if (a.placed && a.u != b.u) w.cls = FIN_FRAG_SPLIT;
        else if (a.placed) {
            const uint32_t ea = a.s0 + a.L, eb = b.s0 + b.L;
            w.u = a.u; w.start = a.s0 < b.s0 ? a.s0 : b.s0; w.length = (ea > eb ? ea : eb) - w.start;
            const Geo &F = a.rev ? b : a, &Rv = a.rev ? a : b;
            w.cls = a.rev == b.rev ? FIN_FRAG_TANDEM : F.s0 <= Rv.s0 && F.s0 + F.L <= Rv.s0 + Rv.L ? FIN_FRAG_INWARD : FIN_FRAG_OUTWARD;
        }
        want_cnt[w.cls]++;
        if (w.cls == FIN_FRAG_INWARD) { want_cnt[6] += w.length; const uint64_t q = w.length / bw; want_hist[q < n_bins - 1u ? q : n_bins - 1u]++; }
        w.cls |= bits;
        want[f] = w;
    }
    for (int c = 0; c < 6; c++) MUST(want_cnt[c] >= 8);
    const uint64_t ns = stream.size() / 2;
    MUST(fin_records_fragments(recs.data(), n_reads, stream.data(), ns, k, ends.data(), ends.size(), n_bins, bw, got.data(), got_hist.data(), got_cnt, threads) == FIN_OK);
    MUST(memcmp(got.data(), want.data(), n_frags * sizeof(fin_fragment)) == 0);
    MUST(memcmp(got_hist.data(), want_hist.data(), (size_t)n_bins * 8) == 0 && memcmp(got_cnt, want_cnt, 56) == 0);
    // every output may be NULL; no reads at all
    MUST(fin_records_fragments(recs.data(), n_reads, stream.data(), ns, k, ends.data(), ends.size(), 0, 0, nullptr, nullptr, nullptr, threads) == FIN_OK);
    MUST(fin_records_fragments(nullptr, 0, nullptr, 0, k, ends.data(), ends.size(), n_bins, bw, nullptr, got_hist.data(), got_cnt, threads) == FIN_OK);
    for (uint64_t v : got_hist) MUST(v == 0);
    for (uint64_t v : got_cnt) MUST(v == 0);
    // the refusals
    MUST(fin_records_fragments(recs.data(), n_reads - 1, stream.data(), ns, k, ends.data(), ends.size(), n_bins, bw, got.data(), got_hist.data(), got_cnt, threads) == FIN_EINVAL);
    MUST(fin_records_fragments(recs.data(), n_reads, stream.data(), ns, k, ends.data(), ends.size(), 0, bw, got.data(), got_hist.data(), got_cnt, threads) == FIN_EINVAL);
    MUST(fin_records_fragments(recs.data(), n_reads, stream.data(), ns, k, ends.data(), ends.size(), FIN_FRAG_MAX_BINS + 1, bw, got.data(), got_hist.data(), got_cnt, threads) == FIN_EINVAL);
    MUST(fin_records_fragments(recs.data(), n_reads, stream.data(), ns, k, ends.data(), ends.size(), n_bins, 0, got.data(), got_hist.data(), got_cnt, threads) == FIN_EINVAL);
    MUST(fin_records_fragments(recs.data(), n_reads, stream.data(), ns, 0, ends.data(), ends.size(), n_bins, bw, got.data(), got_hist.data(), got_cnt, threads) == FIN_EINVAL);
    MUST(fin_records_fragments(nullptr, n_reads, stream.data(), ns, k, ends.data(), ends.size(), n_bins, bw, got.data(), got_hist.data(), got_cnt, threads) == FIN_EINVAL);
    MUST(fin_records_fragments(recs.data(), n_reads, nullptr, ns, k, ends.data(), ends.size(), n_bins, bw, got.data(), got_hist.data(), got_cnt, threads) == FIN_EINVAL);
    MUST(fin_records_fragments(recs.data(), n_reads, stream.data(), ns, k, nullptr, ends.size(), n_bins, bw, got.data(), got_hist.data(), got_cnt, threads) == FIN_EINVAL);
    MUST(fin_records_fragments(recs.data(), n_reads, stream.data(), ns - 1, k, ends.data(), ends.size(), n_bins, bw, got.data(), got_hist.data(), got_cnt, threads) == FIN_EINVAL);
    MUST(fin_records_fragments(recs.data(), n_reads, stream.data(), ns, k, ends.data(), 1, n_bins, bw, got.data(), got_hist.data(), got_cnt, threads) == FIN_EINVAL);   // unitigs 1 and 2 are outside now
    {
        std::vector<fin_read_record> bad = recs;
        uint64_t r = 0;
        while ((bad[r].meta >> 16) != 1u) r++;
        bad[r].off0 = (uint32_t)lens[bad[r].u];   // a record whose k-mers do not lie inside its unitig
        MUST(fin_records_fragments(bad.data(), n_reads, stream.data(), ns, k, ends.data(), ends.size(), n_bins, bw, got.data(), got_hist.data(), got_cnt, threads) == FIN_EINVAL);
        bad = recs; bad[r].meta = 3u << 16;
        MUST(fin_records_fragments(bad.data(), n_reads, stream.data(), ns, k, ends.data(), ends.size(), n_bins, bw, got.data(), got_hist.data(), got_cnt, threads) == FIN_EINVAL);
        const std::vector<int64_t> down = {10, 5, 20};
        MUST(fin_records_fragments(recs.data(), n_reads, stream.data(), ns, k, down.data(), down.size(), n_bins, bw, got.data(), got_hist.data(), got_cnt, threads) == FIN_EINVAL);
    }
    // the effective lengths under the histogram just made: buffers of exactly n entries
    const std::vector<uint64_t> ref = {0, 1, 8, 9, 40, 44, 45, 100, 6000, 1ull << 40, ~0ull};
    std::vector<double> eff(ref.size(), -1.0);
    if (bw == 1u) {
        MUST(fin_effective_lengths(want_hist.data(), n_bins, 1, ref.data(), ref.size(), eff.data()) == FIN_OK);
        for (size_t i = 0; i < ref.size(); i++) {
            uint64_t s0 = 0, s1 = 0;
            for (uint64_t j = 0; j + 1 < n_bins && j <= ref[i]; j++) { s0 += want_hist[j]; s1 += j * want_hist[j]; }
            const double len = (double)ref[i], v = s0 ? len + 1.0 - (double)s1 / (double)s0 : len;
            MUST(eff[i] == (s0 && v >= 1.0 ? v : len));
        }
        MUST(fin_effective_lengths(want_hist.data(), n_bins, 1, nullptr, 0, nullptr) == FIN_OK);
    }
    MUST(fin_effective_lengths(want_hist.data(), n_bins, bw == 1u ? 2u : bw, ref.data(), ref.size(), eff.data()) == FIN_EINVAL);
    MUST(fin_effective_lengths(want_hist.data(), n_bins, 0, ref.data(), ref.size(), eff.data()) == FIN_EINVAL);
    MUST(fin_effective_lengths(nullptr, n_bins, 1, ref.data(), ref.size(), eff.data()) == FIN_EINVAL);
    MUST(fin_effective_lengths(want_hist.data(), 0, 1, ref.data(), ref.size(), eff.data()) == FIN_EINVAL);
    MUST(fin_effective_lengths(want_hist.data(), FIN_FRAG_MAX_BINS + 1, 1, ref.data(), ref.size(), eff.data()) == FIN_EINVAL);
    MUST(fin_effective_lengths(want_hist.data(), n_bins, 1, nullptr, ref.size(), eff.data()) == FIN_EINVAL);
    MUST(fin_effective_lengths(want_hist.data(), n_bins, 1, ref.data(), ref.size(), nullptr) == FIN_EINVAL);
    return 0;
}

int main() {
    for (uint32_t n_bins : {1u, 2u, 64u, 4096u})
        for (uint32_t bw : {1u, 3u, 1000u})
            for (int threads : {1, 7})
                if (run(n_bins, bw, threads)) return 1;
    printf("ok\n");
    return 0;
}
