// The host twins of the record consumers (finito_amd/csrc/fin_records_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program: no
// Python, no device, no HIP -- that one translation unit is all it takes.  From the repository root:
//   g++ -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=c++17 -fopenmp -o /tmp/asan_records tools/asan_records.cpp finito_amd/csrc/fin_records_host.cpp
//   /tmp/asan_records
// Hand-made records -- one slot, eight positions, gaps that touch, overlap and reach both ends, fewer slots than k - 1, both strands, searched (kind 0) and
// all-absent (kind 2) reads between them -- go through every function of that file with output buffers of exactly the size the header asks for, at k = 1, 4 and
// 31, with one thread and with three.  Every result is held against the pairs fin_expand_records makes of the same records.  It prints "ok" and exits 0 when the
// calls gave what they must and the sanitizers reported nothing.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/finito_amd.h"

#define MUST(x) do { if (!(x)) { fprintf(stderr, "failed: %s (line %d, k = %d, threads = %d)\n", #x, __LINE__, k, threads); return 1; } } while (0)

static fin_read_record kind1(uint32_t u, uint32_t off0, uint32_t nk, bool rev, std::vector<uint32_t> Es) {
    fin_read_record R{u, off0, (uint32_t)Es.size() | (rev ? 1u << 8 : 0u) | (1u << 16), nk, 0, 0};
    for (size_t e = 0; e < Es.size(); e++) (e < 4 ? R.Es : R.Es2) |= (uint64_t)Es[e] << (16 * (e & 3));
    return R;
}

static int run(int k, int threads) {
    const uint32_t K = (uint32_t)k, n_unitigs = 4, n_colors = 70, W = 2;
    std::vector<int64_t> ends(n_unitigs);
    for (uint32_t u = 0; u < n_unitigs; u++) ends[u] = (int64_t)(u + 1) * (200 + K);   // 201 k-mers each
    const uint32_t big = 3 * K + 30, tiny = K > 2 ? K - 2 : 1;
    std::vector<fin_read_record> recs;
    std::vector<int32_t> stream;
    const std::vector<std::vector<int32_t>> searched = {{2, 3, 2, 4, -1, -1, 2, 9, 2, 8}, {-1, -1, 3, 100, 3, 100, 0, 0}, {}, {1, 5}};
    for (uint32_t rep = 0; rep < 120; rep++) {
        for (int rev = 0; rev < 2; rev++) {
            const uint32_t u = (rep + rev) % n_unitigs, off = rep % 50;
            recs.push_back(kind1(u, off, 1, rev, {0}));                                    // one slot, absent
            recs.push_back(kind1(u, 200, 1, rev, {}));                                     // one slot, found, the unitig's last k-mer
            recs.push_back(kind1(u, off, 40, rev, {2, 7, 12, 17, 22, 27, 32, 37}));        // eight positions
            recs.push_back(kind1(u, off, big, rev, {10, 10 + K}));                         // two gaps that touch
            recs.push_back(kind1(u, off, big, rev, {10, 11, 12, 12 + K, 12 + 2 * K}));     // gaps that overlap (k > 1) and touch
            recs.push_back(kind1(u, 201 - big, big, rev, {0, big + K - 2}));               // both ends: the first slot, and the last ones clamped
            recs.push_back(kind1(u, off, tiny, rev, {K - 1}));                             // fewer slots than k - 1 (k > 2): one position takes them all
            recs.push_back(kind1(u, off, tiny, rev, {}));
            const auto& s = searched[(rep + rev) % searched.size()];                      // a searched read and an all-absent one between them
            recs.push_back(fin_read_record{0, 0, 0, (uint32_t)(s.size() / 2), 0, 0});
            stream.insert(stream.end(), s.begin(), s.end());
            recs.push_back(fin_read_record{0, 0, 2u << 16, rep % 4, 0, 0});
        }
    }
    const uint64_t n = recs.size(), n_stream = stream.size() / 2;
    uint64_t n_kmers = 0;
    std::vector<uint32_t> nks(n);
    for (uint64_t r = 0; r < n; r++) { nks[r] = recs[r].nk; n_kmers += recs[r].nk; }

    // ---- the pairs: everything below is held against them
    std::vector<int32_t> pairs(2 * n_kmers);
    uint64_t n_pos = 0, found = 0;
    MUST(fin_expand_records(recs.data(), n, stream.data(), n_stream, k, pairs.data(), &n_pos, threads) == FIN_OK);
    for (uint64_t i = 0; i < n_kmers; i++) found += pairs[2 * i] != -1;
    MUST(found == n_pos && found > 0 && found < n_kmers);
    MUST(fin_expand_records(recs.data(), n, stream.data(), n_stream - 1, k, pairs.data(), nullptr, threads) == FIN_EINVAL);   // not this record set's stream
    {   // the third record of the set, forward strand: the slots the rule says
        uint64_t at = 2;   // (two reads of one slot in front of it)
        for (uint32_t sl = 0; sl < 40; sl++) {
            bool gap = false;
            for (uint32_t E = 2; E <= 37; E += 5) gap = gap || (sl <= E && E <= sl + K - 1);
            MUST(gap ? pairs[2 * (at + sl)] == -1 && pairs[2 * (at + sl) + 1] == -1 : pairs[2 * (at + sl)] == (int32_t)recs[2].u && pairs[2 * (at + sl) + 1] == (int32_t)(recs[2].off0 + sl));
        }
    }

    // ---- the profile, the bitmap, the depth
    const uint64_t total_len = (uint64_t)ends.back();
    std::vector<uint64_t> counts(n_unitigs), want_counts(n_unitigs, 0), bits((total_len + 63) / 64), want_bits((total_len + 63) / 64, 0);
    std::vector<uint32_t> depth(total_len), want_depth(total_len, 0);
    for (uint64_t i = 0; i < n_kmers; i++) {
        if (pairs[2 * i] < 0) continue;
        const uint64_t u = (uint64_t)pairs[2 * i], g = (u ? (uint64_t)ends[u - 1] : 0) + (uint64_t)pairs[2 * i + 1];
        want_counts[u]++; want_bits[g >> 6] |= 1ull << (g & 63); want_depth[g]++;
    }
    MUST(fin_records_unitig_counts(recs.data(), n, stream.data(), n_stream, k, n_unitigs, counts.data(), threads) == FIN_OK && counts == want_counts);
    MUST(fin_records_cover(recs.data(), n, stream.data(), n_stream, k, ends.data(), n_unitigs, bits.data(), threads) == FIN_OK && bits == want_bits);
    MUST(fin_records_depth(recs.data(), n, stream.data(), n_stream, k, ends.data(), n_unitigs, depth.data(), threads) == FIN_OK && depth == want_depth);
    MUST(fin_records_unitig_counts(recs.data(), n, stream.data(), n_stream, k, 2, counts.data(), threads) == FIN_EINVAL);   // unitigs 2 and 3 are outside

    // ---- segments, and the pairs back from them
    std::vector<uint64_t> seg_offs(n + 1);
    uint64_t n_segs = 0;
    MUST(fin_records_segments(recs.data(), n, stream.data(), n_stream, k, seg_offs.data(), nullptr, 0, &n_segs, threads) == FIN_ELIMIT && n_segs > n / 2);
    std::vector<fin_segment> segs(n_segs);
    MUST(fin_records_segments(recs.data(), n, stream.data(), n_stream, k, seg_offs.data(), segs.data(), n_segs, &n_segs, threads) == FIN_OK && seg_offs[n] == n_segs);
    std::vector<int32_t> back(2 * n_kmers);
    uint64_t back_pos = 0;
    MUST(fin_expand_segments(seg_offs.data(), segs.data(), n, nks.data(), back.data(), &back_pos, threads) == FIN_OK && back == pairs && back_pos == n_pos);

    // ---- summaries: n_found and span straight from the pairs, n_segments and longest from the segments
    std::vector<fin_read_summary> sums(n);
    MUST(fin_records_read_summaries(recs.data(), n, stream.data(), n_stream, k, sums.data(), threads) == FIN_OK);
    std::vector<uint32_t> found_of(n, 0);
    for (uint64_t r = 0, at = 0; r < n; at += nks[r], r++) {
        uint32_t first = 0, last = 0, longest = 0;
        for (uint32_t i = 0; i < nks[r]; i++) if (pairs[2 * (at + i)] != -1) { if (!found_of[r]) first = i; last = i; found_of[r]++; }
        for (uint64_t s = seg_offs[r]; s < seg_offs[r + 1]; s++) longest = std::max(longest, (uint32_t)std::abs(segs[s].len));
        MUST(sums[r].n_found == found_of[r] && sums[r].span == (found_of[r] ? last - first + 1 : 0) && sums[r].n_segments == seg_offs[r + 1] - seg_offs[r] && sums[r].longest == longest);
    }

    // ---- classes: label u % 3, unitig 3 unlabelled
    const std::vector<uint32_t> labels = {0, 1, 2, FIN_NO_LABEL};
    std::vector<fin_read_class> cls(n);
    MUST(fin_records_read_classes(recs.data(), n, stream.data(), n_stream, k, labels.data(), n_unitigs, cls.data(), threads) == FIN_OK);
    for (uint64_t r = 0, at = 0; r < n; at += nks[r], r++) {
        uint32_t c[3] = {0, 0, 0};
        for (uint32_t i = 0; i < nks[r]; i++) if (pairs[2 * (at + i)] >= 0 && pairs[2 * (at + i)] < 3) c[pairs[2 * (at + i)]]++;
        const uint32_t best = std::max(c[0], std::max(c[1], c[2]));
        MUST(cls[r].n_labelled == c[0] + c[1] + c[2] && cls[r].n_best == best && (best ? c[cls[r].label] == best : cls[r].label == FIN_NO_LABEL));
    }

    // ---- colour rows, per read and per fragment: unitig u has colours u and 64 + u, unitig 3 none
    std::vector<uint64_t> color_bits((size_t)n_unitigs * W, 0);
    for (uint32_t u = 0; u < 3; u++) { color_bits[u * W] = 1ull << u; color_bits[u * W + 1] = 1ull << u; }
    std::vector<uint64_t> rows(n * W), frows(n / 2 * W);
    std::vector<fin_read_pseudo> heads(n);
    std::vector<fin_pair_pseudo> fheads(n / 2);
    MUST(fin_records_pseudoalign(recs.data(), n, stream.data(), n_stream, k, color_bits.data(), n_unitigs, n_colors, 0, rows.data(), heads.data(), threads) == FIN_OK);
    MUST(n % 2 == 0 && fin_records_pseudoalign_paired(recs.data(), n, stream.data(), n_stream, k, color_bits.data(), n_unitigs, n_colors, 0, FIN_PAIR_ANY, frows.data(),
                                                      fheads.data(), threads) == FIN_OK);
    std::vector<uint64_t> want_row(n, 0);   // (permille 0: every colour met)
    std::vector<uint32_t> colored_of(n, 0);
    for (uint64_t r = 0, at = 0; r < n; at += nks[r], r++) {
        for (uint32_t i = 0; i < nks[r]; i++) if (pairs[2 * (at + i)] >= 0 && pairs[2 * (at + i)] < 3) { want_row[r] |= 1ull << pairs[2 * (at + i)]; colored_of[r]++; }
        MUST(heads[r].n_found == found_of[r] && heads[r].n_colored == colored_of[r] && rows[r * W] == want_row[r] && rows[r * W + 1] == want_row[r]);
        MUST(heads[r].n_colors == 2 * (uint32_t)__builtin_popcountll(want_row[r]));
    }
    for (uint64_t f = 0; f < n / 2; f++) {
        MUST(fheads[f].n_found == found_of[2 * f] + found_of[2 * f + 1] && fheads[f].n_colored == colored_of[2 * f] + colored_of[2 * f + 1] && fheads[f].n_colored_first == colored_of[2 * f]);
        MUST(frows[f * W] == (want_row[2 * f] | want_row[2 * f + 1]) && frows[f * W + 1] == frows[f * W]);
    }
    MUST(fin_records_pseudoalign_paired(recs.data(), n - 1, stream.data(), n_stream, k, color_bits.data(), n_unitigs, n_colors, 0, FIN_PAIR_ANY, frows.data(), fheads.data(),
                                        threads) == FIN_EINVAL);   // an odd number of reads
    return 0;
}

int main() {
    for (int k : {1, 4, 31}) for (int threads : {1, 3}) if (run(k, threads)) return 1;
    puts("ok");
    return 0;
}
