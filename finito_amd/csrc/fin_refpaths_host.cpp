// fin_refpaths_host.cpp -- the host twins of fin_refpaths.hip (include/finito_amd.h: REFERENCE COORDINATES, fin_segments_check, fin_segments_window_depth,
// fin_segments_lift_variants): the definitions, no device, no HIP header.  Plain C++ with OpenMP, threads over sequences:
// tools/asan_refpaths.cpp compiles this file beside fin_records_host.cpp (fin_host_threads).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/finito_amd.h"

namespace {
void say(char* err, size_t errlen, const char* fmt, unsigned long long a = 0, unsigned long long b = 0) {
    if (err && errlen) snprintf(err, errlen, fmt, a, b);
}
inline uint64_t abs_len(int32_t len) { return len < 0 ? (uint64_t)(-(int64_t)len) : (uint64_t)len; }
inline uint64_t u_start(const int64_t* ends, int64_t u) { return u ? (uint64_t)ends[u - 1] : 0; }

// the threads' cuts over n_seqs sequences
int threads_for(uint64_t n_seqs, int n_threads) {
    int T = n_threads > 0 ? n_threads : fin_host_threads();
    if ((uint64_t)T > n_seqs) T = (int)(n_seqs ? n_seqs : 1);
    return T < 1 ? 1 : T;
}

// g[i] of the variants, checked: inside the index, strictly ascending
int variant_places(const fin_variant* v, uint64_t n, const int64_t* ends, uint64_t n_unitigs, std::vector<uint64_t>& g, char* err, size_t errlen) {
    g.resize((size_t)n);
    for (uint64_t i = 0; i < n; i++) {
        if (v[i].u >= n_unitigs || u_start(ends, v[i].u) + v[i].off >= (uint64_t)ends[v[i].u]) { say(err, errlen, "variant %llu lies outside the index", i); return FIN_EINVAL; }
        g[(size_t)i] = u_start(ends, v[i].u) + v[i].off;
        if (i && g[(size_t)i] <= g[(size_t)i - 1]) { say(err, errlen, "variant %llu does not ascend: the variants are strictly ascending in start(u) + off", i); return FIN_EINVAL; }
    }
    return FIN_OK;
}
}  // namespace

int fin_segments_check(const uint32_t* seq_nk, const uint64_t* seg_offs, const fin_segment* segs, uint64_t n_seqs, int k, const int64_t* unitig_ends,
                       uint64_t n_unitigs, char* err, size_t errlen) {
    if (k < 1 || (n_seqs && (!seq_nk || !seg_offs)) || (n_unitigs && !unitig_ends)) { say(err, errlen, "null or bad argument"); return FIN_EINVAL; }
    if (n_seqs == 0) return FIN_OK;
    int64_t prev = 0;
    for (uint64_t u = 0; u < n_unitigs; u++) { if (unitig_ends[u] < prev) { say(err, errlen, "unitig_ends descends at unitig %llu", u); return FIN_EINVAL; } prev = unitig_ends[u]; }
    if (seg_offs[0] != 0) { say(err, errlen, "seg_offs does not begin at 0"); return FIN_EINVAL; }
    for (uint64_t s = 0; s < n_seqs; s++) if (seg_offs[s + 1] < seg_offs[s]) { say(err, errlen, "seg_offs descends at sequence %llu", s); return FIN_EINVAL; }
    if (seg_offs[n_seqs] && !segs) { say(err, errlen, "null segments"); return FIN_EINVAL; }
    for (uint64_t s = 0; s < n_seqs; s++) {
        uint64_t next = 0;   // the first slot a segment of this sequence may begin at
        for (uint64_t i = seg_offs[s]; i < seg_offs[s + 1]; i++) {
            const fin_segment& g = segs[i];
            const uint64_t n = abs_len(g.len);
            if (g.u < 0 || (uint64_t)g.u >= n_unitigs) { say(err, errlen, "segment %llu (sequence %llu): unitig number outside the index", i, s); return FIN_EINVAL; }
            if (n == 0) { say(err, errlen, "segment %llu (sequence %llu): len is 0", i, s); return FIN_EINVAL; }
            if ((uint64_t)g.slot + n > seq_nk[s]) { say(err, errlen, "segment %llu (sequence %llu): it leaves the sequence's slots", i, s); return FIN_EINVAL; }
            if (g.slot < next) { say(err, errlen, "segment %llu (sequence %llu): it overlaps or precedes the segment before it", i, s); return FIN_EINVAL; }
            next = (uint64_t)g.slot + n;
            const uint64_t ulen = (uint64_t)unitig_ends[g.u] - u_start(unitig_ends, g.u);
            const uint64_t nk = ulen >= (uint64_t)k ? ulen - (uint64_t)k + 1 : 0;
            const bool ok = g.off >= 0 && (g.len > 0 ? (uint64_t)g.off + n <= nk : (uint64_t)g.off >= n - 1 && (uint64_t)g.off < nk);
            if (!ok) { say(err, errlen, "segment %llu (sequence %llu): offsets outside the unitig's k-mers", i, s); return FIN_EINVAL; }
        }
    }
    return FIN_OK;
}

int fin_segments_window_depth(const uint32_t* seq_nk, const uint64_t* seg_offs, const fin_segment* segs, uint64_t n_seqs, int k, const int64_t* unitig_ends,
                              uint64_t n_unitigs, const uint32_t* depth, uint32_t window, uint32_t min_depth, uint64_t* win_offs_out, fin_ref_window* out, uint64_t cap,
                              uint64_t* n_windows, int n_threads, char* err, size_t errlen) {
    if (n_windows) *n_windows = 0;
    if (window == 0) { say(err, errlen, "window is at least 1"); return FIN_EINVAL; }
    if (const int rc = fin_segments_check(seq_nk, seg_offs, segs, n_seqs, k, unitig_ends, n_unitigs, err, errlen)) return rc;
    if (n_seqs && seg_offs[n_seqs] && !depth) { say(err, errlen, "null depth"); return FIN_EINVAL; }
    std::vector<uint64_t> wo((size_t)n_seqs + 1, 0);
    for (uint64_t s = 0; s < n_seqs; s++) wo[(size_t)s + 1] = wo[(size_t)s] + ((uint64_t)seq_nk[s] + window - 1) / window;
    const uint64_t W = wo[(size_t)n_seqs];
    if (n_windows) *n_windows = W;
    if (W > cap || (W && !out)) { say(err, errlen, "window buffer too small: room for %llu windows, %llu needed", cap, W); return FIN_ELIMIT; }
    if (win_offs_out) memcpy(win_offs_out, wo.data(), ((size_t)n_seqs + 1) * 8);
    const uint32_t floor = min_depth ? min_depth : 1u;
    const int T = threads_for(n_seqs, n_threads);
#pragma omp parallel for schedule(dynamic, 1) num_threads(T)
    for (int64_t s = 0; s < (int64_t)n_seqs; s++) {
        fin_ref_window* const w = out + wo[(size_t)s];
        if (wo[(size_t)s + 1] > wo[(size_t)s]) memset(w, 0, (size_t)(wo[(size_t)s + 1] - wo[(size_t)s]) * sizeof(fin_ref_window));
        for (uint64_t i = seg_offs[s]; i < seg_offs[s + 1]; i++) {
            const fin_segment& g = segs[i];
            const uint64_t n = abs_len(g.len), g0 = u_start(unitig_ends, g.u) + (uint64_t)g.off;
            for (uint64_t j = 0; j < n; j++) {
                const uint32_t d = depth[g.len > 0 ? g0 + j : g0 - j];
                fin_ref_window& o = w[((uint64_t)g.slot + j) / window];
                o.depth_sum += d; o.in_graph++; o.covered += d >= floor ? 1u : 0u;
            }
        }
    }
    return FIN_OK;
}

int fin_segments_lift_variants(const uint32_t* seq_nk, const uint64_t* seg_offs, const fin_segment* segs, uint64_t n_seqs, int k, const int64_t* unitig_ends,
                               uint64_t n_unitigs, const fin_variant* vars, uint64_t n, fin_ref_variant* out, uint64_t cap, uint64_t* n_out, int n_threads, char* err,
                               size_t errlen) {
    if (n_out) *n_out = 0;
    if (n && !vars) { say(err, errlen, "null variants"); return FIN_EINVAL; }
    if (const int rc = fin_segments_check(seq_nk, seg_offs, segs, n_seqs, k, unitig_ends, n_unitigs, err, errlen)) return rc;
    std::vector<uint64_t> g;
    if (const int rc = variant_places(vars, n, unitig_ends, n_unitigs, g, err, errlen)) return rc;
    if (n_seqs == 0 || n == 0) return FIN_OK;
    // a segment's variants: [j0, j1) of g[], those inside its base interval [x0, x0 + n + k - 2]
    auto range = [&](const fin_segment& sg, uint64_t& x0, uint64_t& j0, uint64_t& j1) {
        const uint64_t m = abs_len(sg.len), st = u_start(unitig_ends, sg.u) + (uint64_t)sg.off;
        x0 = sg.len > 0 ? st : st - (m - 1);
        const uint64_t x1 = x0 + m + (uint64_t)k - 2;
        j0 = (uint64_t)(std::lower_bound(g.begin(), g.end(), x0) - g.begin());
        j1 = (uint64_t)(std::upper_bound(g.begin(), g.end(), x1) - g.begin());
    };
    const int T = threads_for(n_seqs, n_threads);
    std::vector<uint64_t> at((size_t)n_seqs + 1, 0);
#pragma omp parallel for schedule(dynamic, 16) num_threads(T)
    for (int64_t s = 0; s < (int64_t)n_seqs; s++) {
        uint64_t c = 0, x0, j0, j1;
        for (uint64_t i = seg_offs[s]; i < seg_offs[s + 1]; i++) { range(segs[i], x0, j0, j1); c += j1 - j0; }
        at[(size_t)s + 1] = c;
    }
    for (uint64_t s = 0; s < n_seqs; s++) at[(size_t)s + 1] += at[(size_t)s];
    const uint64_t total = at[(size_t)n_seqs];
    if (n_out) *n_out = total;
    if (total > cap || (total && !out)) { say(err, errlen, "record buffer too small: room for %llu records, %llu needed", cap, total); return FIN_ELIMIT; }
#pragma omp parallel for schedule(dynamic, 16) num_threads(T)
    for (int64_t s = 0; s < (int64_t)n_seqs; s++) {
        fin_ref_variant* o = out + at[(size_t)s];
        for (uint64_t i = seg_offs[s]; i < seg_offs[s + 1]; i++) {
            const fin_segment& sg = segs[i];
            uint64_t x0, j0, j1;
            range(sg, x0, j0, j1);
            const uint64_t m = abs_len(sg.len);
            for (uint64_t q = 0; q < j1 - j0; q++) {   // descending through g for a reverse segment: pos ascends
                const uint64_t j = sg.len > 0 ? j0 + q : j1 - 1 - q, x = g[(size_t)j] - x0;
                *o++ = fin_ref_variant{(uint32_t)s, (uint32_t)((uint64_t)sg.slot + (sg.len > 0 ? x : m + (uint64_t)k - 2 - x)), (uint32_t)j, sg.len > 0 ? 0u : 1u};
            }
        }
    }
    return FIN_OK;
}
