// fin_fragments_host.cpp -- the host twins of fin_fragments.hip (include/finito_amd.h: FRAGMENT GEOMETRY, fin_records_fragments, fin_effective_lengths; DESIGN.md
// 4.27): the definitions, no device, no HIP header.  Plain C++ with OpenMP: tools/asan_fragments.cpp compiles this file beside fin_records_host.cpp
// (fin_host_threads).  fin_records_fragments reads the definition off a read's EXPANDED slots, whichever kind its record is -- a kind-1 record's are made as
// fin_expand_records makes them (fin_rec_walk.h) --: it is the CPU statement of the definition, not of the kernel's shortcut.
#include <string.h>

#include <vector>

#include "../../include/finito_amd.h"
#include "fin_rec_walk.h"

namespace {
struct Mate { uint32_t u = 0xFFFFFFFFu, s0 = 0, L = 0; bool placed = false, rev = false; };

// rules 1 and 2 of the pileup over the nk slots p of one read.  false: a slot that is neither found nor (-1,-1), a unitig number >= n_unitigs, a k-mer that does not
// lie inside its unitig
bool place_mate(const int32_t* p, uint32_t nk, int k, const int64_t* ends, uint64_t n_unitigs, Mate& m) {
    uint64_t n_found = 0; int64_t u0 = -1, dF = 0, dR = 0; bool okF = true, okR = true;
    for (uint32_t i = 0; i < nk; i++) {
        const int64_t u = p[2 * (size_t)i], off = p[2 * (size_t)i + 1];
        if (u < 0 || off < 0) { if (u != -1) return false; continue; }
        if ((uint64_t)u >= n_unitigs) return false;
        const uint64_t start = u ? (uint64_t)ends[u - 1] : 0, end = (uint64_t)ends[u];
        if (start + (uint64_t)off + (uint64_t)k > end) return false;
        if (n_found == 0) { u0 = u; dF = off - (int64_t)i; dR = off + (int64_t)i; }
        n_found++;
        if (u != u0 || off - (int64_t)i != dF) okF = false;
        if (u != u0 || off + (int64_t)i != dR) okR = false;
    }
    if (n_found < 2 || okF == okR) return true;   // not straight
    const bool rev = okR;
    const uint64_t L = (uint64_t)nk + (uint64_t)k - 1;
    const int64_t s0 = rev ? dR - (int64_t)nk + 1 : dF;
    const uint64_t start = u0 ? (uint64_t)ends[u0 - 1] : 0, end = (uint64_t)ends[u0];
    if (s0 < 0 || start + (uint64_t)s0 + L > end) return true;   // hangs over an end of its unitig
    m.u = (uint32_t)u0; m.s0 = (uint32_t)s0; m.L = (uint32_t)L; m.placed = true; m.rev = rev;
    return true;
}

fin_fragment combine(const Mate& a, const Mate& b) {
    const uint32_t bits = (a.placed && a.rev ? 0x100u : 0u) | (b.placed && b.rev ? 0x200u : 0u) | (a.placed ? 0x400u : 0u) | (b.placed ? 0x800u : 0u);
    if (!a.placed && !b.placed) return fin_fragment{0xFFFFFFFFu, 0u, 0u, FIN_FRAG_NONE | bits};
    if (a.placed != b.placed) { const Mate& m = a.placed ? a : b; return fin_fragment{m.u, m.s0, m.L, FIN_FRAG_ONE | bits}; }
    if (a.u != b.u) return fin_fragment{0xFFFFFFFFu, 0u, 0u, FIN_FRAG_SPLIT | bits};
    const uint64_t ea = (uint64_t)a.s0 + a.L, eb = (uint64_t)b.s0 + b.L;
    const uint32_t start = a.s0 < b.s0 ? a.s0 : b.s0, length = (uint32_t)((ea > eb ? ea : eb) - start);
    uint32_t cls = FIN_FRAG_TANDEM;
    if (a.rev != b.rev) {
        const Mate& F = a.rev ? b : a; const Mate& R = a.rev ? a : b;
        cls = F.s0 <= R.s0 && (uint64_t)F.s0 + F.L <= (uint64_t)R.s0 + R.L ? FIN_FRAG_INWARD : FIN_FRAG_OUTWARD;
    }
    return fin_fragment{a.u, start, length, cls | bits};
}
}  // namespace

int fin_records_fragments(const fin_read_record* recs, uint64_t n_reads, const int32_t* stream_pairs, uint64_t n_stream_pairs, int k, const int64_t* unitig_ends,
                          uint64_t n_unitigs, uint32_t n_bins, uint32_t bin_width, fin_fragment* frags_out, uint64_t* hist_out, uint64_t counters_out[7],
                          int n_threads) {
    if ((n_reads && !recs) || (n_reads & 1u) || k < 1 || (n_stream_pairs && !stream_pairs) || (n_unitigs && !unitig_ends)) return FIN_EINVAL;
    if (hist_out && (n_bins == 0 || n_bins > FIN_FRAG_MAX_BINS || bin_width == 0)) return FIN_EINVAL;
    int64_t prev = 0;
    for (uint64_t u = 0; u < n_unitigs; u++) { if (unitig_ends[u] < prev) return FIN_EINVAL; prev = unitig_ends[u]; }
    const uint64_t n_frags = n_reads / 2;
    int T = n_threads > 0 ? n_threads : fin_host_threads();
    if ((uint64_t)T > n_frags / 1024 + 1) T = (int)(n_frags / 1024 + 1);
    auto lo = [&](int t) { return 2 * (n_frags * (uint64_t)t / (uint64_t)T); };   // a thread's reads: the cuts fall between fragments
    // where each thread's share of the stream begins: only the kind-0 reads have a share
    std::vector<uint64_t> str0((size_t)T + 1, 0);
#pragma omp parallel for schedule(static) num_threads(T)
    for (int t = 0; t < T; t++) {
        uint64_t x = 0;
        for (uint64_t r = lo(t); r < lo(t + 1); r++) if ((recs[r].meta >> 16) == 0u) x += recs[r].nk;
        str0[(size_t)t + 1] = x;
    }
    for (int t = 0; t < T; t++) str0[(size_t)t + 1] += str0[(size_t)t];
    if (str0[(size_t)T] != n_stream_pairs) return FIN_EINVAL;   // records and stream do not belong together
    const size_t nb = hist_out ? n_bins : 0;
    std::vector<uint64_t> part((size_t)T * (nb + 7), 0);   // per thread: its histogram, then its counters
    bool ok = true;
#pragma omp parallel for schedule(static) num_threads(T) reduction(&& : ok)
    for (int t = 0; t < T; t++) {
        uint64_t sp = str0[(size_t)t];
        uint64_t* const h = part.data() + (size_t)t * (nb + 7);
        uint64_t* const c = h + nb;
        std::vector<int32_t> own;   // a kind-1 or kind-2 read's slots
        bool good = true;
        for (uint64_t f = lo(t) / 2; good && f < lo(t + 1) / 2; f++) {
            Mate m[2];
            for (int s = 0; good && s < 2; s++) {
                const fin_read_record& R = recs[2 * f + (uint64_t)s];
                const uint32_t nk = R.nk, kind = R.meta >> 16;
                if (kind > 2u) { good = false; break; }
                const int32_t* p = nullptr;
                if (kind == 0u) { p = stream_pairs + 2 * sp; sp += nk; }
                else {
                    own.assign((size_t)nk * 2, -1);
                    if (kind == 1u) {
                        const bool rev = (R.meta >> 8) & 1u;
                        (void)fin_rec_stretches(nk, R.meta & 0xFFu, (uint32_t)R.Es, (uint32_t)(R.Es >> 32), (uint32_t)R.Es2, (uint32_t)(R.Es2 >> 32), (uint32_t)k,
                                                [&](uint32_t, uint32_t from, uint32_t to) {
                            for (uint32_t sl = from; sl < to; sl++) {
                                const uint32_t i = rev ? nk - 1u - sl : sl;
                                own[2 * (size_t)i] = (int32_t)R.u; own[2 * (size_t)i + 1] = (int32_t)(R.off0 + sl);
                            }
                        });
                    }
                    p = own.data();
                }
                good = place_mate(p, nk, k, unitig_ends, n_unitigs, m[s]);
            }
            if (!good) break;
            const fin_fragment fr = combine(m[0], m[1]);
            if (frags_out) frags_out[f] = fr;
            const uint32_t cls = fr.cls & 0xFFu;
            c[cls]++;
            if (cls == FIN_FRAG_INWARD) {
                c[6] += fr.length;
                if (nb) { const uint32_t q = fr.length / bin_width; h[q < n_bins - 1u ? q : n_bins - 1u]++; }
            }
        }
        ok = good && ok;
    }
    if (!ok) return FIN_EINVAL;
    for (size_t b = 0; b < nb; b++) { uint64_t s = 0; for (int t = 0; t < T; t++) s += part[(size_t)t * (nb + 7) + b]; hist_out[b] = s; }
    if (counters_out) for (size_t c = 0; c < 7; c++) { uint64_t s = 0; for (int t = 0; t < T; t++) s += part[(size_t)t * (nb + 7) + nb + c]; counters_out[c] = s; }
    return FIN_OK;
}

int fin_effective_lengths(const uint64_t* hist, uint32_t n_bins, uint32_t bin_width, const uint64_t* ref_len, uint64_t n, double* out) {
    if (!hist || n_bins == 0 || n_bins > FIN_FRAG_MAX_BINS || bin_width != 1u || (n && (!ref_len || !out))) return FIN_EINVAL;
    // S0(l), S1(l) over the bins below the last one, which means "this much or more"
    const uint32_t nb = n_bins - 1u;
    std::vector<uint64_t> S0(nb), S1(nb);
    uint64_t s0 = 0, s1 = 0;
    for (uint32_t j = 0; j < nb; j++) { s0 += hist[j]; s1 += (uint64_t)j * hist[j]; S0[j] = s0; S1[j] = s1; }
    for (uint64_t i = 0; i < n; i++) {
        const double len = (double)ref_len[i];
        out[i] = len;
        if (nb == 0) continue;
        const uint64_t m = ref_len[i] < (uint64_t)(nb - 1u) ? ref_len[i] : (uint64_t)(nb - 1u);   // min(ref_len, n_bins - 2)
        if (S0[m] == 0) continue;
        const double v = len + 1.0 - (double)S1[m] / (double)S0[m];   // one division: the same bits wherever it runs
        if (v >= 1.0) out[i] = v;
    }
    return FIN_OK;
}
