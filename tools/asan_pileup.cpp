// fin_records_pileup (finito_amd/csrc/fin_records_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program: no Python, no device,
// no HIP.  From the repository root:
//   g++ -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=c++17 -fopenmp -o /tmp/asan_pileup tools/asan_pileup.cpp finito_amd/csrc/fin_records_host.cpp
//   /tmp/asan_pileup
// A random text of four unitigs; reads spelled from it on both strands with 0 .. 3 substitutions, an N, lower case, reads at the first and the last base of a
// unitig, reads of one slot, reads shorter than k, an empty read -- as kind-1 records with exactly their substitutions as positions, as kind-0 reads with their
// pairs in the stream (straight, a mosaic of two unitigs, a repeated pair), and as kind-2 reads -- go through fin_records_pileup with output buffers of exactly
// the size the header asks for, at k = 4 and 31, with one thread and with three, each output also left out in turn.  The result is held against a count made here
// from the reads' known places.  It prints "ok" and exits 0 when the calls gave what they must and the sanitizers reported nothing.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/finito_amd.h"

#define MUST(x) do { if (!(x)) { fprintf(stderr, "failed: %s (line %d, k = %d, threads = %d)\n", #x, __LINE__, k, threads); return 1; } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd(uint32_t n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state % n); }

static std::string revcomp(const std::string& s) {
    std::string r(s.rbegin(), s.rend());
    for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c == 'a' ? 't' : c == 'c' ? 'g' : c == 'g' ? 'c' : c == 't' ? 'a' : c;
    return r;
}

static int run(int k, int threads) {
    const uint32_t K = (uint32_t)k, n_unitigs = 4, max_mm = 2;
    std::vector<int64_t> ends(n_unitigs);
    for (uint32_t u = 0; u < n_unitigs; u++) ends[u] = (int64_t)(u + 1) * (150 + K);
    const uint64_t total = (uint64_t)ends.back();
    std::vector<uint8_t> concat(total);
    for (auto& c : concat) c = (uint8_t)rnd(4);
    std::vector<fin_read_record> recs;
    std::vector<int32_t> stream;
    std::string bases;
    std::vector<uint64_t> offsets = {0};
    std::vector<uint32_t> want_cover(total, 0), want_alt(4 * total, 0);
    uint64_t want_n[4] = {0, 0, 0, 0};
    auto push = [&](const std::string& read) { bases += read; offsets.push_back(bases.size()); };
    for (uint32_t rep = 0; rep < 300; rep++) {
        const uint32_t u = rep % n_unitigs, ulen = 150 + K, L = rep % 7 == 0 ? K : rep % 7 == 1 ? K + 1 : K + 1 + rnd(100), nk = L - K + 1;
        const uint32_t off0 = rep % 5 == 0 ? 0 : rep % 5 == 1 ? ulen - L : rnd(ulen - L + 1), n_sub = rep % 4;
        const bool rev = rep & 1, as_rec = rep % 3 != 0, lower = rep % 11 == 0;
        const uint64_t g0 = (u ? (uint64_t)ends[u - 1] : 0) + off0;
        std::string s(L, 'A');
        for (uint32_t j = 0; j < L; j++) s[j] = "ACGT"[concat[g0 + j]];
        std::vector<uint32_t> Es;
        for (uint32_t e = 0; e < n_sub; e++) {   // ascending positions, each base changed once
            const uint32_t lo = Es.empty() ? 0 : Es.back() + 1;
            if (lo >= L) break;
            const uint32_t E = lo + rnd(L - lo);
            s[E] = "ACGT"[(concat[g0 + E] + 1 + rnd(3)) % 4];
            Es.push_back(E);
        }
        const bool with_n = !as_rec && rep % 13 == 0 && L > 2;   // (the fast path leaves no record for a read with another letter)
        if (with_n) { bool is_sub = false; for (uint32_t E : Es) is_sub = is_sub || E == 1; if (is_sub) for (size_t e = 0; e < Es.size(); e++) if (Es[e] == 1) { Es.erase(Es.begin() + (long)e); break; } s[1] = 'N'; }
        // the slots the substitutions and the N leave
        std::vector<int32_t> p(2 * (size_t)nk, -1);
        uint32_t n_found = 0;
        for (uint32_t sl = 0; sl < nk; sl++) {
            bool gap = with_n && sl <= 1 && 1 <= sl + K - 1;
            for (uint32_t E : Es) gap = gap || (sl <= E && E <= sl + K - 1);
            if (!gap) { const uint32_t i = rev ? nk - 1 - sl : sl; p[2 * (size_t)i] = (int32_t)u; p[2 * (size_t)i + 1] = (int32_t)(off0 + sl); n_found++; }
        }
        if (as_rec) {
            fin_read_record R{u, off0, (uint32_t)Es.size() | (rev ? 1u << 8 : 0u) | (1u << 16), nk, 0, 0};
            for (size_t e = 0; e < Es.size(); e++) (e < 4 ? R.Es : R.Es2) |= (uint64_t)Es[e] << (16 * (e & 3));
            recs.push_back(R);
        } else {
            recs.push_back(fin_read_record{0, 0, 0, nk, 0, 0});
            stream.insert(stream.end(), p.begin(), p.end());
        }
        std::string read = rev ? revcomp(s) : s;
        if (lower) for (char& c : read) c = (char)(c | 0x20);
        push(read);
        const uint32_t outcome = n_found < 2 ? FIN_PILEUP_NOT_STRAIGHT : Es.size() > max_mm ? FIN_PILEUP_TOO_MANY : FIN_PILEUP_KEPT;
        want_n[outcome]++;
        if (outcome == FIN_PILEUP_KEPT) {
            for (uint32_t j = 0; j < L; j++) want_cover[g0 + j]++;
            for (uint32_t E : Es) { uint32_t b = 0; while ("ACGT"[b] != s[E]) b++; want_alt[4 * (g0 + E) + b]++; }
        }
        // between them: a mosaic and a repeated pair (not straight), an all-absent read, a read shorter than k, an empty read
        if (rep % 10 == 0) {
            recs.push_back(fin_read_record{0, 0, 0, 3, 0, 0});
            const int32_t mosaic[6] = {0, 5, 0, 6, 1, 7}, twice[6] = {2, 9, 2, 9, -1, -1};
            stream.insert(stream.end(), rep % 20 ? twice : mosaic, (rep % 20 ? twice : mosaic) + 6);
            push(std::string(K + 2, 'C')); want_n[FIN_PILEUP_NOT_STRAIGHT]++;
            recs.push_back(fin_read_record{0, 0, 2u << 16, 2, 0, 0}); push(std::string(K + 1, 'G')); want_n[FIN_PILEUP_NOT_STRAIGHT]++;
            recs.push_back(fin_read_record{0, 0, 0, 0, 0, 0}); push(std::string(K - 1, 'T')); want_n[FIN_PILEUP_NOT_STRAIGHT]++;
            recs.push_back(fin_read_record{0, 0, 0, 0, 0, 0}); push(""); want_n[FIN_PILEUP_NOT_STRAIGHT]++;
        }
    }
    // a straight read that hangs over the end of its unitig: slots (1, ulen - K - 1), (1, ulen - K) and an absent one
    {
        const int32_t hang[6] = {1, (int32_t)(150 - 1), 1, (int32_t)150, -1, -1};
        recs.push_back(fin_read_record{0, 0, 0, 3, 0, 0}); stream.insert(stream.end(), hang, hang + 6); push(std::string(K + 2, 'A')); want_n[FIN_PILEUP_OFF_UNITIG]++;
    }
    const uint64_t n = recs.size(), n_stream = stream.size() / 2;
    const std::vector<char> exact(bases.begin(), bases.end());   // (a buffer of exactly the reads' bytes, no terminator behind it)
    std::vector<uint32_t> cover(total), alt(4 * total);
    uint64_t counters[4];
    auto call = [&](uint32_t* c, uint32_t* a, uint64_t* cn, uint64_t ns, uint32_t mm) {
        return fin_records_pileup(recs.data(), n, stream.data(), ns, k, exact.data(), offsets.data(), ends.data(), n_unitigs, concat.data(), mm, c, a, cn, threads);
    };
    MUST(call(cover.data(), alt.data(), counters, n_stream, max_mm) == FIN_OK);
    MUST(cover == want_cover && alt == want_alt);
    for (int c = 0; c < 4; c++) MUST(counters[c] == want_n[c] && want_n[c] > 0);
    std::vector<uint32_t> cover2(total), alt2(4 * total);
    MUST(call(cover2.data(), nullptr, nullptr, n_stream, max_mm) == FIN_OK && cover2 == want_cover);
    MUST(call(nullptr, alt2.data(), nullptr, n_stream, max_mm) == FIN_OK && alt2 == want_alt);
    MUST(call(nullptr, nullptr, counters, n_stream, 255) == FIN_OK && counters[FIN_PILEUP_TOO_MANY] == 0);
    MUST(call(cover2.data(), alt2.data(), counters, n_stream - 1, max_mm) == FIN_EINVAL);   // not this record set's stream
    MUST(call(cover2.data(), alt2.data(), counters, n_stream, 256) == FIN_EINVAL);
    {
        std::vector<fin_read_record> bad = recs;
        for (auto& R : bad) if ((R.meta >> 16) == 1u && (R.meta & 0xFFu) == 0u) { R.u = n_unitigs; break; }   // (a record with found slots)
        MUST(fin_records_pileup(bad.data(), n, stream.data(), n_stream, k, exact.data(), offsets.data(), ends.data(), n_unitigs, concat.data(), max_mm, cover2.data(),
                                alt2.data(), counters, threads) == FIN_EINVAL);
    }
    return 0;
}

int main() {
    for (int k : {4, 31}) for (int threads : {1, 3}) if (run(k, threads)) return 1;
    puts("ok");
    return 0;
}
