// fin_records_host.cpp -- the host twins of the record consumers (include/finito_amd.h): everything that turns records, segments and a stream into results on
// the CPU.  Plain C++17 with OpenMP: no HIP header, no device call -- the file compiles, links and runs by itself (tools/asan_records.cpp).  What a kind-1
// record means is taken from fin_rec_walk.h, the one statement of the gap rule that the device kernels take it from too: no function here works out a gap.
#include <sched.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/finito_amd.h"
#include "fin_format.h"
#include "fin_host.h"
#include "fin_rec_walk.h"
#include "fin_taxa.h"

static_assert(sizeof(fin_read_record) == sizeof(FinFastRec) && offsetof(fin_read_record, nk) == 12 && offsetof(FinFastRec, nk) == 12 &&
              offsetof(fin_read_record, Es) == 16 && offsetof(FinFastRec, Es) == 16 && offsetof(fin_read_record, Es2) == 24 && offsetof(FinFastRec, Es2) == 24,
              "the public record is the device's, byte for byte: the halves of Es and Es2 are the four position words a lane loads");

namespace {
// the gaps and the found stretches of a kind-1 record (fin_rec_walk.h)
template <class F>
void rec_gaps(const fin_read_record& R, int k, F&& emit) {
    fin_rec_gaps(R.nk, R.meta & 0xFFu, (uint32_t)R.Es, (uint32_t)(R.Es >> 32), (uint32_t)R.Es2, (uint32_t)(R.Es2 >> 32), (uint32_t)k, emit);
}
template <class F>
uint32_t rec_stretches(const fin_read_record& R, int k, F&& emit) {
    return fin_rec_stretches(R.nk, R.meta & 0xFFu, (uint32_t)R.Es, (uint32_t)(R.Es >> 32), (uint32_t)R.Es2, (uint32_t)(R.Es2 >> 32), (uint32_t)k, emit);
}

// A read set cut into T chunks of consecutive reads, a chunk per thread: chunk t is reads [lo(t), hi(t)).  `unit` = 2: the cuts fall between fragments
struct Chunks {
    int T;
    uint64_t n, unit;
    std::vector<uint64_t> str0;   // after stream(): the stream pair chunk t's share begins at, [T + 1]
    Chunks(uint64_t n_reads, int n_threads, uint64_t unit_ = 1) : T(n_threads > 0 ? n_threads : fin_host_threads()), n(n_reads / unit_), unit(unit_) {
        if ((uint64_t)T > n / 1024 + 1) T = (int)(n / 1024 + 1);
    }
    uint64_t lo(int t) const { return unit * (n * (uint64_t)t / (uint64_t)T); }
    uint64_t hi(int t) const { return lo(t + 1); }
    // body(t) for every chunk, in parallel: true when every one of them said true
    template <class B>
    bool run(B&& body) const {
        bool ok = true;
#pragma omp parallel for num_threads(T) schedule(static) reduction(&& : ok)
        for (int t = 0; t < T; t++) ok = body(t) && ok;
        return ok;
    }
    // where each chunk's share of a total begins: the sums of per_read(r) over the chunks in front of it, [T + 1]
    template <class G>
    std::vector<uint64_t> starts(G&& per_read) const {
        std::vector<uint64_t> s((size_t)T + 1, 0);
        (void)run([&](int t) { uint64_t x = 0; for (uint64_t r = lo(t); r < hi(t); r++) x += per_read(r); s[(size_t)t + 1] = x; return true; });
        for (int t = 0; t < T; t++) s[(size_t)t + 1] += s[(size_t)t];
        return s;
    }
    // ... of the stream, which only the kind-0 reads have a share of.  FIN_EINVAL: records and stream do not belong together
    int stream(const fin_read_record* recs, uint64_t n_stream_pairs) {
        str0 = starts([&](uint64_t r) { return (recs[r].meta >> 16) == 0u ? (uint64_t)recs[r].nk : 0ull; });
        return str0[(size_t)T] == n_stream_pairs ? FIN_OK : FIN_EINVAL;
    }
};

// the canonical segmentation of one read's slots (include/finito_amd.h): emit(u, off, slot, len) per segment, in slot order.  false: a pair that is neither
// found nor (-1,-1)
template <class F>
bool segment_slots(const int32_t* p, uint32_t nk, F&& emit) {
    int lp = 0;            // link(i - 1)
    uint32_t head = 0; bool in = false; int dir = 0;   // the open segment: its head slot, the sign of its internal links (0: one slot so far)
    auto close = [&](uint32_t end) {
        if (!in) return;
        const uint32_t n = end - head;
        emit(p[2 * head], p[2 * head + 1], head, dir < 0 ? -(int32_t)n : (int32_t)n);
        in = false;
    };
    for (uint32_t i = 0; i < nk; i++) {
        const int32_t u = p[2 * i], off = p[2 * i + 1];
        if (u < 0) {
            if (u != -1) return false;
            close(i); lp = 0;
            continue;
        }
        int l = 0;
        if (i && p[2 * i - 2] == u) { const int64_t d = (int64_t)off - (int64_t)p[2 * i - 1]; l = d == 1 ? 1 : d == -1 ? -1 : 0; }
        if (l == 0 || (lp != 0 && lp != l)) { close(i); head = i; in = true; dir = 0; }
        else dir = l;
        lp = l;
    }
    close(nk);
    return true;
}
// the found stretches of a kind-1 record as segments, in slot order: strand A's own order, or mirrored when strand A is the reverse strand
template <class F>
void segment_record(const fin_read_record& R, int k, F&& emit) {
    const uint32_t nk = R.nk;
    const bool rev = (R.meta >> 8) & 1u;
    uint32_t from[9], to[9];
    const uint32_t n = rec_stretches(R, k, [&](uint32_t s, uint32_t f, uint32_t t) { from[s] = f; to[s] = t; });
    for (uint32_t s = 0; s < n; s++) {
        if (!rev) emit((int32_t)R.u, (int32_t)(R.off0 + from[s]), from[s], (int32_t)(to[s] - from[s]));
        else { const uint32_t q = n - 1u - s, len = to[q] - from[q]; emit((int32_t)R.u, (int32_t)(R.off0 + to[q] - 1u), nk - to[q], len == 1u ? 1 : -(int32_t)len); }
    }
}
// read r's segments, whichever kind it is: emit(u, off, slot, len); `sp` moves over a kind-0 read's share of the stream.  false: as segment_slots
template <class F>
bool read_segments(const fin_read_record& R, const int32_t* stream_pairs, uint64_t& sp, int k, F&& emit) {
    const uint32_t kind = R.meta >> 16;
    bool good = true;
    if (kind == 0u) { good = segment_slots(stream_pairs + 2 * sp, R.nk, emit); sp += R.nk; }
    else if (kind == 1u) segment_record(R, k, emit);
    return good;
}

// a read's or a fragment's segments as (unitig, slots), tallied under the colour matrix: cnt[colour] += slots, for every colour of the unitig
struct ColorTally {
    uint32_t W;
    std::vector<std::pair<uint32_t, uint32_t>> segs;
    std::vector<uint64_t> cnt;
    uint64_t n_found = 0, n_colored = 0, n_first = 0;   // n_first: the coloured slots of segs[0 .. n_first_segs)
    explicit ColorTally(uint32_t W_) : W(W_), cnt((size_t)W_ * 64) {}
    void tally(const uint64_t* bits, size_t n_first_segs) {
        std::fill(cnt.begin(), cnt.end(), 0);
        n_found = n_colored = n_first = 0;
        for (size_t q = 0; q < segs.size(); q++) {
            const auto& sg = segs[q];
            n_found += sg.second;
            const uint64_t* row = bits + (uint64_t)sg.first * W;
            bool ne = false;
            for (uint32_t w = 0; w < W; w++) {
                uint64_t x = row[w];
                if (x) ne = true;
                for (; x; x &= x - 1) cnt[(size_t)w * 64 + (size_t)__builtin_ctzll(x)] += sg.second;
            }
            if (ne) { n_colored += sg.second; if (q < n_first_segs) n_first += sg.second; }
        }
    }
    // row[0 .. W) = the colours with at least permille thousandths of the coloured slots (none when !keep); returns how many
    uint32_t row(uint32_t permille, bool keep, uint64_t* out) const {
        uint32_t pc = 0;
        for (uint32_t w = 0; w < W; w++) {
            uint64_t o = 0;
            if (keep) for (uint32_t q = 0; q < 64u; q++) { const uint64_t c = cnt[(size_t)w * 64 + q]; if (c >= 1 && 1000ull * c >= (uint64_t)permille * n_colored) o |= 1ull << q; }
            out[w] = o; pc += (uint32_t)__builtin_popcountll(o);
        }
        return pc;
    }
};

// what fin_records_cover and fin_records_depth share: the places of the found k-mers as ranges of text positions.  mark(g_lo, g_hi) for offsets
// [off_lo, off_hi) of unitig u, each the first base of a found k-mer that must lie whole inside the unitig; false: a place outside the index or a pair that is
// neither found nor (-1,-1)
template <class M>
bool chunk_places(const Chunks& C, int t, const fin_read_record* recs, const int32_t* stream_pairs, int k, const int64_t* unitig_ends, uint64_t n_unitigs, M&& mark) {
    uint64_t sp = C.str0[(size_t)t];
    bool good = true;
    auto range = [&](uint64_t u, uint64_t off_lo, uint64_t off_hi) {
        if (u >= n_unitigs) { good = false; return; }
        const uint64_t start = u ? (uint64_t)unitig_ends[u - 1] : 0, end = (uint64_t)unitig_ends[u];
        if (start + off_hi - 1 + (uint64_t)k > end) { good = false; return; }
        mark(start + off_lo, start + off_hi);
    };
    for (uint64_t r = C.lo(t); r < C.hi(t) && good; r++) {
        const fin_read_record& R = recs[r];
        const uint32_t nk = R.nk, kind = R.meta >> 16;
        if (kind == 0u) {
            const int32_t* const src = stream_pairs + 2 * sp;
            for (uint32_t i = 0; i < nk; i++) {
                const int32_t u = src[2 * i], off = src[2 * i + 1];
                if (u >= 0 && off >= 0) range((uint64_t)u, (uint64_t)off, (uint64_t)off + 1);
                else if (u != -1) good = false;
            }
            sp += nk;
        } else if (kind == 1u) {
            (void)rec_stretches(R, k, [&](uint32_t, uint32_t from, uint32_t to) { range(R.u, (uint64_t)R.off0 + from, (uint64_t)R.off0 + to); });
        }
    }
    return good;
}
}  // namespace

extern "C" {

// (here, not in fin_capi.cpp, so that this file links by itself)
int fin_host_threads(void) {
    int n = 1;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char a[64]; long long per = 0;
        if (fscanf(f, "%63s %lld", a, &per) == 2 && strcmp(a, "max") != 0 && per > 0) {
            long long q = atoll(a) / per;
            if (q >= 1 && q < n) n = (int)q;
        }
        fclose(f);
    }
    int cap = 64;
    if (const char* e = getenv("FINITO_THREADS")) { int v = atoi(e); if (v > 0) cap = v; }
    if (n > cap) n = cap;
    return n < 1 ? 1 : n;
}

// the pairs fin_search_batch delivers, from records + stream.  A chunk of reads per thread: first where each chunk's pairs and stream begin, then the pairs
int fin_expand_records(const fin_read_record* recs, uint64_t n_reads, const int32_t* stream_pairs, uint64_t n_stream_pairs, int k, int32_t* pairs_out,
                       uint64_t* n_positive, int n_threads) {
    if ((n_reads && (!recs || !pairs_out)) || k < 1 || (n_stream_pairs && !stream_pairs)) return FIN_EINVAL;
    Chunks C(n_reads, n_threads);
    if (C.stream(recs, n_stream_pairs)) return FIN_EINVAL;
    const std::vector<uint64_t> out0 = C.starts([&](uint64_t r) { return (uint64_t)recs[r].nk; });
    std::vector<uint64_t> pos((size_t)C.T, 0);
    (void)C.run([&](int t) {
        uint64_t o = out0[(size_t)t], sp = C.str0[(size_t)t], found = 0;
        for (uint64_t r = C.lo(t); r < C.hi(t); r++) {
            const fin_read_record& R = recs[r];
            const uint32_t nk = R.nk, kind = R.meta >> 16;
            int32_t* const dst = pairs_out + 2 * o;
            if (kind == 0u) {
                memcpy(dst, stream_pairs + 2 * sp, (size_t)nk * 8);
                for (uint32_t i = 0; i < nk; i++) found += dst[2 * i] != -1;
                sp += nk;
            } else if (kind == 2u) {
                for (uint32_t i = 0; i < 2 * nk; i++) dst[i] = -1;
            } else {
                // one run: slot sl of strand A is (u, off0 + sl) unless it lies in a gap; the reverse strand's slots mirror
                const bool rev = (R.meta >> 8) & 1u;
                for (uint32_t i = 0; i < nk; i++) { const uint32_t sl = rev ? nk - 1u - i : i; dst[2 * i] = (int32_t)R.u; dst[2 * i + 1] = (int32_t)(R.off0 + sl); }
                uint32_t gaps = 0;
                rec_gaps(R, k, [&](uint32_t lo, uint32_t hi_excl) {
                    for (uint32_t sl = lo; sl < hi_excl; sl++) { const uint32_t i = rev ? nk - 1u - sl : sl; dst[2 * i] = -1; dst[2 * i + 1] = -1; }
                    gaps += hi_excl - lo;
                });
                found += nk - gaps;
            }
            o += nk;
        }
        pos[(size_t)t] = found;
        return true;
    });
    if (n_positive) { uint64_t f = 0; for (uint64_t x : pos) f += x; *n_positive = f; }
    return FIN_OK;
}

// the segments of fin_segments.hip from records + stream, the pairs never made.  A chunk of reads per thread: first how many segments each chunk has, then
// the segments
int fin_records_segments(const fin_read_record* recs, uint64_t n_reads, const int32_t* stream_pairs, uint64_t n_stream_pairs, int k, uint64_t* seg_offs_out,
                         fin_segment* segs_out, uint64_t seg_cap, uint64_t* n_segments, int n_threads) {
    if ((n_reads && !recs) || k < 1 || (n_stream_pairs && !stream_pairs) || !seg_offs_out) return FIN_EINVAL;
    if (n_segments) *n_segments = 0;
    Chunks C(n_reads, n_threads);
    if (C.stream(recs, n_stream_pairs)) return FIN_EINVAL;
    std::vector<uint64_t> seg0((size_t)C.T + 1, 0);
    auto pass = [&](int t, bool write) {
        uint64_t sp = C.str0[(size_t)t], sg = write ? seg0[(size_t)t] : 0;
        auto emit = [&](int32_t u, int32_t off, uint32_t slot, int32_t len) { if (write) segs_out[sg] = fin_segment{u, off, slot, len}; sg++; };
        for (uint64_t r = C.lo(t); r < C.hi(t); r++) {
            if (write) seg_offs_out[r] = sg;
            if (!read_segments(recs[r], stream_pairs, sp, k, emit)) return false;
        }
        if (!write) seg0[(size_t)t + 1] = sg;
        return true;
    };
    if (!C.run([&](int t) { return pass(t, false); })) return FIN_EINVAL;
    for (int t = 0; t < C.T; t++) seg0[(size_t)t + 1] += seg0[(size_t)t];
    const uint64_t total = seg0[(size_t)C.T];
    if (n_segments) *n_segments = total;
    if (total > seg_cap || (total && !segs_out)) return total > seg_cap ? FIN_ELIMIT : FIN_EINVAL;
    (void)C.run([&](int t) { return pass(t, true); });
    seg_offs_out[n_reads] = total;
    return FIN_OK;
}

// fin_search_batch's pairs from segments.  Every read is checked before anything of it is written
int fin_expand_segments(const uint64_t* seg_offs, const fin_segment* segs, uint64_t n_reads, const uint32_t* nk_per_read, int32_t* pairs_out, uint64_t* n_positive,
                        int n_threads) {
    if (!seg_offs || (n_reads && !nk_per_read)) return FIN_EINVAL;
    for (uint64_t r = 0; r < n_reads; r++) if (seg_offs[r + 1] < seg_offs[r]) return FIN_EINVAL;
    if (n_reads && seg_offs[n_reads] > seg_offs[0] && !segs) return FIN_EINVAL;
    const Chunks C(n_reads, n_threads);
    const bool ok = C.run([&](int t) {   // every segment checked
        for (uint64_t r = C.lo(t); r < C.hi(t); r++) {
            const uint64_t nk = nk_per_read[r];
            uint64_t next = 0;   // the first slot a segment may begin at
            for (uint64_t s = seg_offs[r]; s < seg_offs[r + 1]; s++) {
                const fin_segment& S = segs[s];
                const uint64_t n = S.len < 0 ? (uint64_t)(-(int64_t)S.len) : (uint64_t)S.len;
                if (n == 0 || S.u < 0 || S.off < 0 || S.slot < next || (uint64_t)S.slot + n > nk) return false;
                if (S.len < 0 ? (int64_t)S.off - (int64_t)(n - 1) < 0 : (int64_t)S.off + (int64_t)(n - 1) > 0x7FFFFFFFll) return false;
                next = (uint64_t)S.slot + n;
            }
        }
        return true;
    });
    if (!ok) return FIN_EINVAL;
    const std::vector<uint64_t> out0 = C.starts([&](uint64_t r) { return (uint64_t)nk_per_read[r]; });   // where each chunk's pairs begin
    if (out0[(size_t)C.T] && !pairs_out) return FIN_EINVAL;
    std::vector<uint64_t> pos((size_t)C.T, 0);
    (void)C.run([&](int t) {
        uint64_t o = out0[(size_t)t], found = 0;
        for (uint64_t r = C.lo(t); r < C.hi(t); r++) {
            const uint64_t nk = nk_per_read[r];
            int32_t* const dst = pairs_out + 2 * o;
            for (uint64_t i = 0; i < 2 * nk; i++) dst[i] = -1;
            for (uint64_t s = seg_offs[r]; s < seg_offs[r + 1]; s++) {
                const fin_segment& S = segs[s];
                const int32_t step = S.len < 0 ? -1 : 1;
                const uint32_t n = (uint32_t)(S.len < 0 ? -(int64_t)S.len : (int64_t)S.len);   // (checked above: 1 .. nk)
                for (uint32_t j = 0; j < n; j++) { dst[2 * (S.slot + j)] = S.u; dst[2 * (S.slot + j) + 1] = S.off + step * (int32_t)j; }
                found += n;
            }
            o += nk;
        }
        pos[(size_t)t] = found;
        return true;
    });
    if (n_positive) { uint64_t f = 0; for (uint64_t x : pos) f += x; *n_positive = f; }
    return FIN_OK;
}

// the summaries of fin_readsum.hip from records + stream, over the segments segment_slots / segment_record make: n_found is the sum of their lengths, span
// runs from the first one's slot to the last one's end
int fin_records_read_summaries(const fin_read_record* recs, uint64_t n_reads, const int32_t* stream_pairs, uint64_t n_stream_pairs, int k, fin_read_summary* out,
                               int n_threads) {
    if ((n_reads && (!recs || !out)) || k < 1 || (n_stream_pairs && !stream_pairs)) return FIN_EINVAL;
    Chunks C(n_reads, n_threads);
    if (C.stream(recs, n_stream_pairs)) return FIN_EINVAL;
    const bool ok = C.run([&](int t) {
        uint64_t sp = C.str0[(size_t)t];
        bool good = true;
        for (uint64_t r = C.lo(t); r < C.hi(t) && good; r++) {
            fin_read_summary S{0, 0, 0, 0};
            uint32_t first = 0, end = 0;
            good = read_segments(recs[r], stream_pairs, sp, k, [&](int32_t, int32_t, uint32_t slot, int32_t len) {
                const uint32_t n = (uint32_t)(len < 0 ? -(int64_t)len : (int64_t)len);
                if (S.n_segments == 0) first = slot;
                S.n_found += n; S.n_segments++; if (n > S.longest) S.longest = n;
                end = slot + n;
            });
            S.span = end - first;
            out[r] = S;
        }
        return good;
    });
    return ok ? FIN_OK : FIN_EINVAL;
}

// the classes of fin_classify.hip from records + stream, over the same segments: a segment of |len| slots in unitig u is |len| votes for labels[u]
int fin_records_read_classes(const fin_read_record* recs, uint64_t n_reads, const int32_t* stream_pairs, uint64_t n_stream_pairs, int k,
                             const uint32_t* unitig_labels, uint64_t n_unitigs, fin_read_class* out, int n_threads) {
    if ((n_reads && (!recs || !out)) || k < 1 || (n_stream_pairs && !stream_pairs) || (n_unitigs && !unitig_labels)) return FIN_EINVAL;
    Chunks C(n_reads, n_threads);
    if (C.stream(recs, n_stream_pairs)) return FIN_EINVAL;
    const bool ok = C.run([&](int t) {
        uint64_t sp = C.str0[(size_t)t];
        bool good = true;
        std::vector<std::pair<uint32_t, uint32_t>> votes;   // (label, slots) per segment, then sorted by label
        for (uint64_t r = C.lo(t); r < C.hi(t) && good; r++) {
            votes.clear();
            good = read_segments(recs[r], stream_pairs, sp, k, [&](int32_t u, int32_t, uint32_t, int32_t len) {
                if ((uint64_t)(uint32_t)u >= n_unitigs) { good = false; return; }
                const uint32_t L = unitig_labels[(uint32_t)u];
                if (L != FIN_NO_LABEL) votes.push_back({L, (uint32_t)(len < 0 ? -(int64_t)len : (int64_t)len)});
            }) && good;
            std::sort(votes.begin(), votes.end());
            fin_read_class K{FIN_NO_LABEL, 0, 0, 0};
            for (size_t i = 0; i < votes.size();) {   // ascending labels: a later label wins only with a larger count
                uint32_t c = 0; size_t j = i;
                for (; j < votes.size() && votes[j].first == votes[i].first; j++) c += votes[j].second;
                K.n_labelled += c;
                if (c > K.n_best) { K.n_second = K.n_best; K.n_best = c; K.label = votes[i].first; }
                else if (c > K.n_second) K.n_second = c;
                i = j;
            }
            out[r] = K;
        }
        return good;
    });
    return ok ? FIN_OK : FIN_EINVAL;
}

// the read taxa of fin_taxa.hip from records + stream, over the same segments: a segment of |len| slots in unitig u is |len| votes for labels[u]; the rule
// itself is fin_taxa_call's (fin_taxa_host.cpp)
int fin_records_read_taxa(const fin_read_record* recs, uint64_t n_reads, const int32_t* stream_pairs, uint64_t n_stream_pairs, int k, const uint32_t* unitig_labels,
                          uint64_t n_unitigs, const uint32_t* parent, uint64_t n_taxa, uint32_t min_found, uint32_t confidence_permille, fin_read_taxon* out,
                          int n_threads) {
    if ((n_reads && (!recs || !out)) || k < 1 || (n_stream_pairs && !stream_pairs) || (n_unitigs && !unitig_labels) || !parent) return FIN_EINVAL;
    if (n_taxa == 0 || n_taxa > 0x80000000ull || confidence_permille > 1000u || fin_taxa_first_bad_parent(parent, n_taxa) != n_taxa) return FIN_EINVAL;
    for (uint64_t u = 0; u < n_unitigs; u++) if (unitig_labels[u] != FIN_NO_LABEL && (uint64_t)unitig_labels[u] >= n_taxa) return FIN_EINVAL;
    Chunks C(n_reads, n_threads);
    if (C.stream(recs, n_stream_pairs)) return FIN_EINVAL;
    const bool ok = C.run([&](int t) {
        uint64_t sp = C.str0[(size_t)t];
        bool good = true;
        std::vector<std::pair<uint32_t, uint32_t>> votes;   // (taxon, slots) per segment
        for (uint64_t r = C.lo(t); r < C.hi(t) && good; r++) {
            votes.clear();
            good = read_segments(recs[r], stream_pairs, sp, k, [&](int32_t u, int32_t, uint32_t, int32_t len) {
                if ((uint64_t)(uint32_t)u >= n_unitigs) { good = false; return; }
                const uint32_t L = unitig_labels[(uint32_t)u];
                if (L != FIN_NO_LABEL) votes.push_back({L, (uint32_t)(len < 0 ? -(int64_t)len : (int64_t)len)});
            }) && good;
            out[r] = fin_taxa_call(votes, parent, recs[r].nk, min_found, confidence_permille);
        }
        return good;
    });
    return ok ? FIN_OK : FIN_EINVAL;
}

// the rows and heads of fin_col_pseudo_kernel from records + stream, over the same segments: a segment of |len| slots in unitig u is |len| counts for every
// colour of u
int fin_records_pseudoalign(const fin_read_record* recs, uint64_t n_reads, const int32_t* stream_pairs, uint64_t n_stream_pairs, int k, const uint64_t* bits,
                            uint64_t n_unitigs, uint32_t n_colors, uint32_t permille, uint64_t* rows_out, fin_read_pseudo* heads_out, int n_threads) {
    if ((n_reads && (!recs || !rows_out || !heads_out)) || k < 1 || (n_stream_pairs && !stream_pairs) || (n_unitigs && !bits)) return FIN_EINVAL;
    if (n_colors == 0 || n_colors > FIN_MAX_COLORS) return FIN_ELIMIT;
    if (permille > 1000u) return FIN_EINVAL;
    const uint32_t W = (n_colors + 63u) / 64u;
    if (colors_first_stray(bits, n_unitigs, n_colors, W) != n_unitigs) return FIN_EINVAL;
    Chunks C(n_reads, n_threads);
    if (C.stream(recs, n_stream_pairs)) return FIN_EINVAL;
    const bool ok = C.run([&](int t) {
        uint64_t sp = C.str0[(size_t)t];
        bool good = true;
        ColorTally Y(W);
        for (uint64_t r = C.lo(t); r < C.hi(t) && good; r++) {
            Y.segs.clear();
            good = read_segments(recs[r], stream_pairs, sp, k, [&](int32_t u, int32_t, uint32_t, int32_t len) {
                if ((uint64_t)(uint32_t)u >= n_unitigs) { good = false; return; }
                Y.segs.push_back({(uint32_t)u, (uint32_t)(len < 0 ? -(int64_t)len : (int64_t)len)});
            }) && good;
            Y.tally(bits, 0);
            const uint32_t pc = Y.row(permille, true, rows_out + r * W);
            heads_out[r] = fin_read_pseudo{(uint32_t)Y.n_found, (uint32_t)Y.n_colored, pc, 0};
        }
        return good;
    });
    return ok ? FIN_OK : FIN_EINVAL;
}

// the definition of fin_paired.hip over the two mates' segments: fin_records_pseudoalign with a fragment's segments pooled and the first mate's coloured slots
// kept apart.  The chunks are cut between fragments
int fin_records_pseudoalign_paired(const fin_read_record* recs, uint64_t n_reads, const int32_t* stream_pairs, uint64_t n_stream_pairs, int k, const uint64_t* bits,
                                   uint64_t n_unitigs, uint32_t n_colors, uint32_t permille, uint32_t mode, uint64_t* rows_out, fin_pair_pseudo* heads_out, int n_threads) {
    const uint64_t nf = n_reads / 2;
    if ((n_reads && !recs) || (nf && (!rows_out || !heads_out)) || k < 1 || (n_stream_pairs && !stream_pairs) || (n_unitigs && !bits)) return FIN_EINVAL;
    if (n_colors == 0 || n_colors > FIN_MAX_COLORS) return FIN_ELIMIT;
    if (permille > 1000u || (n_reads & 1u) || (mode != FIN_PAIR_ANY && mode != FIN_PAIR_BOTH)) return FIN_EINVAL;
    const uint32_t W = (n_colors + 63u) / 64u;
    if (colors_first_stray(bits, n_unitigs, n_colors, W) != n_unitigs) return FIN_EINVAL;
    Chunks C(n_reads, n_threads, 2);
    if (C.stream(recs, n_stream_pairs)) return FIN_EINVAL;
    const bool ok = C.run([&](int t) {
        uint64_t sp = C.str0[(size_t)t];
        bool good = true;
        ColorTally Y(W);   // (the first mate's segments first)
        for (uint64_t f = C.lo(t) / 2; f < C.hi(t) / 2 && good; f++) {
            Y.segs.clear();
            size_t n_first_segs = 0;
            for (uint64_t r = 2 * f; r < 2 * f + 2; r++) {
                good = read_segments(recs[r], stream_pairs, sp, k, [&](int32_t u, int32_t, uint32_t, int32_t len) {
                    if ((uint64_t)(uint32_t)u >= n_unitigs) { good = false; return; }
                    Y.segs.push_back({(uint32_t)u, (uint32_t)(len < 0 ? -(int64_t)len : (int64_t)len)});
                }) && good;
                if (r == 2 * f) n_first_segs = Y.segs.size();
            }
            Y.tally(bits, n_first_segs);
            const uint32_t pc = Y.row(permille, mode == FIN_PAIR_ANY || (Y.n_first != 0 && Y.n_colored != Y.n_first), rows_out + f * W);
            heads_out[f] = fin_pair_pseudo{(uint32_t)Y.n_found, (uint32_t)Y.n_colored, pc, (uint32_t)Y.n_first};
        }
        return good;
    });
    return ok ? FIN_OK : FIN_EINVAL;
}

// the profile of fin_hits.hip from records + stream, without the pairs.  A chunk of reads per thread; with more than one thread the adds are atomic
int fin_records_unitig_counts(const fin_read_record* recs, uint64_t n_reads, const int32_t* stream_pairs, uint64_t n_stream_pairs, int k, uint64_t n_unitigs,
                              uint64_t* counts_out, int n_threads) {
    if ((n_reads && !recs) || k < 1 || (n_stream_pairs && !stream_pairs) || (n_unitigs && !counts_out)) return FIN_EINVAL;
    for (uint64_t u = 0; u < n_unitigs; u++) counts_out[u] = 0;
    Chunks C(n_reads, n_threads);
    if (C.stream(recs, n_stream_pairs)) return FIN_EINVAL;
    const int T = C.T;
    const bool ok = C.run([&](int t) {
        uint64_t sp = C.str0[(size_t)t];
        bool good = true;
        auto add = [&](uint64_t u, uint64_t n) {
            if (u >= n_unitigs) { good = false; return; }
            if (T == 1) counts_out[u] += n;
            else __atomic_fetch_add(counts_out + u, n, __ATOMIC_RELAXED);
        };
        for (uint64_t r = C.lo(t); r < C.hi(t) && good; r++) {
            const fin_read_record& R = recs[r];
            const uint32_t nk = R.nk, kind = R.meta >> 16;
            if (kind == 0u) {
                const int32_t* const src = stream_pairs + 2 * sp;
                for (uint32_t i = 0; i < nk;) {   // a run of slots in one unitig: one add
                    const int32_t u = src[2 * i];
                    uint32_t j = i + 1;
                    while (j < nk && src[2 * j] == u) j++;
                    if (u >= 0) add((uint64_t)u, j - i);
                    else if (u != -1) good = false;
                    i = j;
                }
                sp += nk;
            } else if (kind == 1u) {
                uint32_t gaps = 0;
                rec_gaps(R, k, [&](uint32_t lo, uint32_t hi_excl) { gaps += hi_excl - lo; });
                if (nk - gaps) add(R.u, nk - gaps);
            }
        }
        return good;
    });
    return ok ? FIN_OK : FIN_EINVAL;
}

// the bitmap of fin_cover.hip from records + stream, the pairs never made.  A chunk of reads per thread; with more than one thread the words are ORed atomically
int fin_records_cover(const fin_read_record* recs, uint64_t n_reads, const int32_t* stream_pairs, uint64_t n_stream_pairs, int k, const int64_t* unitig_ends,
                      uint64_t n_unitigs, uint64_t* bits_out, int n_threads) {
    if ((n_reads && !recs) || k < 1 || (n_stream_pairs && !stream_pairs) || (n_unitigs && (!unitig_ends || !bits_out))) return FIN_EINVAL;
    int64_t prev = 0;
    for (uint64_t u = 0; u < n_unitigs; u++) { if (unitig_ends[u] < prev) return FIN_EINVAL; prev = unitig_ends[u]; }
    const uint64_t total_len = (uint64_t)prev, n_words = (total_len + 63) / 64;
    for (uint64_t w = 0; w < n_words; w++) bits_out[w] = 0;
    Chunks C(n_reads, n_threads);
    if (C.stream(recs, n_stream_pairs)) return FIN_EINVAL;
    const int T = C.T;
    const bool ok = C.run([&](int t) {
        return chunk_places(C, t, recs, stream_pairs, k, unitig_ends, n_unitigs, [&](uint64_t g0, uint64_t g1) {
            for (uint64_t w = g0 >> 6; (w << 6) < g1; w++) {
                const uint64_t wb = w << 6, lo = g0 > wb ? g0 : wb, hi = g1 < wb + 64 ? g1 : wb + 64;
                const uint64_t m = (~0ull >> (64 - (hi - lo))) << (lo - wb);
                if (T == 1) bits_out[w] |= m;
                else __atomic_fetch_or(bits_out + w, m, __ATOMIC_RELAXED);
            }
        });
    });
    return ok ? FIN_OK : FIN_EINVAL;
}

// the depth of fin_depth.hip from records + stream, the pairs never made.  A chunk of reads per thread; with more than one thread the positions are added
// atomically
int fin_records_depth(const fin_read_record* recs, uint64_t n_reads, const int32_t* stream_pairs, uint64_t n_stream_pairs, int k, const int64_t* unitig_ends,
                      uint64_t n_unitigs, uint32_t* depth_out, int n_threads) {
    if ((n_reads && !recs) || k < 1 || (n_stream_pairs && !stream_pairs) || (n_unitigs && (!unitig_ends || !depth_out))) return FIN_EINVAL;
    int64_t prev = 0;
    for (uint64_t u = 0; u < n_unitigs; u++) { if (unitig_ends[u] < prev) return FIN_EINVAL; prev = unitig_ends[u]; }
    const uint64_t total_len = (uint64_t)prev;
    for (uint64_t g = 0; g < total_len; g++) depth_out[g] = 0;
    Chunks C(n_reads, n_threads);
    if (C.stream(recs, n_stream_pairs)) return FIN_EINVAL;
    const int T = C.T;
    const bool ok = C.run([&](int t) {
        return chunk_places(C, t, recs, stream_pairs, k, unitig_ends, n_unitigs, [&](uint64_t g0, uint64_t g1) {
            for (uint64_t g = g0; g < g1; g++) {
                if (T == 1) depth_out[g]++;
                else __atomic_fetch_add(depth_out + g, 1u, __ATOMIC_RELAXED);
            }
        });
    });
    return ok ? FIN_OK : FIN_EINVAL;
}

// the pileup of fin_pileup.hip from records + stream and the reads: the definition of include/finito_amd.h read off a read's pairs, whichever kind its record
// is -- a kind-1 record's are made as fin_expand_records makes them -- and every placed read compared with the text whole.  A chunk of reads per thread; with more
// than one thread the positions are added atomically
int fin_records_pileup(const fin_read_record* recs, uint64_t n_reads, const int32_t* stream_pairs, uint64_t n_stream_pairs, int k, const char* bases,
                       const uint64_t* offsets, const int64_t* unitig_ends, uint64_t n_unitigs, const uint8_t* concat, uint32_t max_mismatch, uint32_t* cover_out,
                       uint32_t* alt_out, uint64_t counters_out[4], int n_threads) {
    if ((n_reads && (!recs || !offsets)) || k < 1 || (n_stream_pairs && !stream_pairs) || (n_unitigs && !unitig_ends) || max_mismatch > 255u) return FIN_EINVAL;
    int64_t prev = 0;
    for (uint64_t u = 0; u < n_unitigs; u++) { if (unitig_ends[u] < prev) return FIN_EINVAL; prev = unitig_ends[u]; }
    const uint64_t total_len = (uint64_t)prev;
    if (total_len && !concat) return FIN_EINVAL;
    if (n_reads && offsets[n_reads] > offsets[0] && !bases) return FIN_EINVAL;
    if (cover_out) for (uint64_t g = 0; g < total_len; g++) cover_out[g] = 0;
    if (alt_out) for (uint64_t g = 0; g < 4 * total_len; g++) alt_out[g] = 0;
    if (counters_out) for (int c = 0; c < 4; c++) counters_out[c] = 0;
    Chunks C(n_reads, n_threads);
    if (C.stream(recs, n_stream_pairs)) return FIN_EINVAL;
    const int T = C.T;
    auto code = [](char ch) -> uint32_t { const char x = (char)(ch & 0xDF); return x == 'A' ? 0u : x == 'C' ? 1u : x == 'G' ? 2u : x == 'T' ? 3u : 4u; };
    auto add32 = [&](uint32_t* p) { if (T == 1) (*p)++; else __atomic_fetch_add(p, 1u, __ATOMIC_RELAXED); };
    std::vector<uint64_t> cnt((size_t)C.T * 4, 0);
    const bool ok = C.run([&](int t) {
        uint64_t sp = C.str0[(size_t)t];
        uint64_t* const my = cnt.data() + (size_t)t * 4;
        std::vector<int32_t> own;   // a kind-1 or kind-2 read's pairs
        for (uint64_t r = C.lo(t); r < C.hi(t); r++) {
            const fin_read_record& R = recs[r];
            const uint32_t nk = R.nk, kind = R.meta >> 16;
            const uint64_t L = offsets[r + 1] - offsets[r];
            if (offsets[r + 1] < offsets[r] || (nk ? L != (uint64_t)nk + (uint64_t)k - 1 : L >= (uint64_t)k) || kind > 2u) return false;
            const int32_t* p = nullptr;
            if (kind == 0u) { p = stream_pairs + 2 * sp; sp += nk; }
            else {
                own.assign((size_t)nk * 2, -1);
                if (kind == 1u) {
                    const bool rev = (R.meta >> 8) & 1u;
                    (void)rec_stretches(R, k, [&](uint32_t, uint32_t from, uint32_t to) {
                        for (uint32_t sl = from; sl < to; sl++) { const uint32_t i = rev ? nk - 1u - sl : sl; own[2 * (size_t)i] = (int32_t)R.u; own[2 * (size_t)i + 1] = (int32_t)(R.off0 + sl); }
                    });
                }
                p = own.data();
            }
            // 1. straight
            uint64_t n_found = 0; int64_t u0 = -1, dF = 0, dR = 0; bool okF = true, okR = true;
            for (uint32_t i = 0; i < nk; i++) {
                const int64_t u = p[2 * (size_t)i], off = p[2 * (size_t)i + 1];
                if (u < 0 || off < 0) { if (u != -1) return false; continue; }
                if ((uint64_t)u >= n_unitigs) return false;
                const uint64_t start = u ? (uint64_t)unitig_ends[u - 1] : 0, end = (uint64_t)unitig_ends[u];
                if (start + (uint64_t)off + (uint64_t)k > end) return false;
                if (n_found == 0) { u0 = u; dF = off - (int64_t)i; dR = off + (int64_t)i; }
                n_found++;
                if (u != u0 || off - (int64_t)i != dF) okF = false;
                if (u != u0 || off + (int64_t)i != dR) okR = false;
            }
            if (n_found < 2 || okF == okR) { my[FIN_PILEUP_NOT_STRAIGHT]++; continue; }
            // 2. placed: strand A at [s0, s0 + L) of u0
            const bool rev = okR;
            const int64_t s0 = rev ? dR - (int64_t)nk + 1 : dF;
            const uint64_t start = u0 ? (uint64_t)unitig_ends[u0 - 1] : 0, end = (uint64_t)unitig_ends[u0];
            if (s0 < 0 || start + (uint64_t)s0 + L > end) { my[FIN_PILEUP_OFF_UNITIG]++; continue; }
            // 3. mismatches: strand position s is read[s] forward, the complement of read[L - 1 - s] reverse
            const uint64_t g0 = start + (uint64_t)s0;
            const char* const rd = bases + offsets[r];
            auto observed = [&](uint64_t s) -> uint32_t { const uint32_t c = code(rd[rev ? L - 1 - s : s]); return rev && c < 4u ? 3u - c : c; };
            uint64_t n_mm = 0;
            for (uint64_t s = 0; s < L; s++) { const uint32_t o = observed(s); if (o < 4u && o != concat[g0 + s]) n_mm++; }
            if (n_mm > max_mismatch) { my[FIN_PILEUP_TOO_MANY]++; continue; }
            // 4. what a kept read adds
            for (uint64_t s = 0; s < L; s++) {
                if (cover_out) add32(cover_out + g0 + s);
                const uint32_t o = observed(s);
                if (alt_out && o < 4u && o != concat[g0 + s]) add32(alt_out + 4 * (g0 + s) + o);
            }
            my[FIN_PILEUP_KEPT]++;
        }
        return true;
    });
    if (!ok) return FIN_EINVAL;
    if (counters_out) for (int t = 0; t < C.T; t++) for (int c = 0; c < 4; c++) counters_out[c] += cnt[(size_t)t * 4 + (size_t)c];
    return FIN_OK;
}

}  // extern "C"
