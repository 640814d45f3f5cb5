// fin_links_host.cpp -- the host twin of fin_links.hip (include/finito_amd.h: LINKS, fin_records_links, fin_link_hash): the definition, no device,
// no HIP header.  Plain C++ with OpenMP: tools/asan_links.cpp compiles this file beside fin_records_host.cpp (fin_host_threads).  fin_records_links reads the
// definition off a read's EXPANDED slots, whichever kind its record is -- a kind-1 record's are made as fin_expand_records makes them (fin_rec_walk.h) --: it is the
// CPU statement of the definition, not of the kernel's shortcut.  Every thread collects the keys of its reads; the keys are sorted and runs of equal keys counted,
// so the result does not depend on the number of threads.
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/finito_amd.h"
#include "fin_linkhash.h"
#include "fin_rec_walk.h"

uint64_t fin_link_hash(uint64_t key) { return fin_link_mix(key); }

namespace {
// the transitions of one read's nk slots p, their keys appended.  false: a transition with an end outside the index
bool read_links(const int32_t* p, uint32_t nk, const int64_t* ends, uint64_t n_unitigs, uint64_t total_len, std::vector<uint64_t>& keys) {
    for (uint32_t i = 1; i < nk; i++) {
        const uint32_t ua = (uint32_t)p[2 * (size_t)i - 2], oa = (uint32_t)p[2 * (size_t)i - 1], ub = (uint32_t)p[2 * (size_t)i], ob = (uint32_t)p[2 * (size_t)i + 1];
        if (ua == 0xFFFFFFFFu || ub == 0xFFFFFFFFu) continue;
        if (ua == ub && (ob == oa + 1u || ob + 1u == oa)) continue;   // straight, either way
        if (ua >= n_unitigs || ub >= n_unitigs) return false;
        const uint64_t ga = (ua ? (uint64_t)ends[ua - 1] : 0) + oa, gb = (ub ? (uint64_t)ends[ub - 1] : 0) + ob;
        if (ga >= total_len || gb >= total_len) return false;
        keys.push_back(fin_link_key((uint32_t)ga, (uint32_t)gb));
    }
    return true;
}
}  // namespace

int fin_records_links(const fin_read_record* recs, uint64_t n_reads, const int32_t* stream_pairs, uint64_t n_stream_pairs, int k, const int64_t* unitig_ends,
                      uint64_t n_unitigs, uint64_t min_count, fin_link* links_out, uint64_t cap_out, uint64_t* n_links, uint64_t counters_out[4], int n_threads) {
    if ((n_reads && !recs) || k < 1 || (n_stream_pairs && !stream_pairs) || (n_unitigs && !unitig_ends) || !n_links) return FIN_EINVAL;
    *n_links = 0;
    int64_t prev = 0;
    for (uint64_t u = 0; u < n_unitigs; u++) { if (unitig_ends[u] < prev) return FIN_EINVAL; prev = unitig_ends[u]; }
    if ((uint64_t)prev >= (1ull << 32)) return FIN_EINVAL;
    const uint64_t total_len = (uint64_t)prev;
    int T = n_threads > 0 ? n_threads : fin_host_threads();
    if ((uint64_t)T > n_reads / 1024 + 1) T = (int)(n_reads / 1024 + 1);
    auto lo = [&](int t) { return n_reads * (uint64_t)t / (uint64_t)T; };
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
    std::vector<std::vector<uint64_t>> part((size_t)T);
    bool ok = true;
#pragma omp parallel for schedule(static) num_threads(T) reduction(&& : ok)
    for (int t = 0; t < T; t++) {
        uint64_t sp = str0[(size_t)t];
        std::vector<int32_t> own;   // a kind-1 or kind-2 read's slots
        bool good = true;
        for (uint64_t r = lo(t); good && r < lo(t + 1); r++) {
            const fin_read_record& R = recs[r];
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
            good = read_links(p, nk, unitig_ends, n_unitigs, total_len, part[(size_t)t]);
        }
        ok = good && ok;
    }
    if (!ok) return FIN_EINVAL;
    std::vector<uint64_t> keys;
    for (int t = 0; t < T; t++) keys.insert(keys.end(), part[(size_t)t].begin(), part[(size_t)t].end());
    std::sort(keys.begin(), keys.end());   // ascending by (g_a, g_b): the canonical order
    const uint64_t need = min_count > 1 ? min_count : 1;
    uint64_t n_distinct = 0, n_kept = 0, n_self = 0;
    for (size_t i = 0; i < keys.size();) {
        size_t j = i;
        while (j < keys.size() && keys[j] == keys[i]) j++;
        const uint32_t ga = (uint32_t)(keys[i] >> 32), gb = (uint32_t)keys[i];
        n_distinct++;
        if (ga == gb) n_self++;
        if ((uint64_t)(j - i) >= need) {
            if (links_out && n_kept < cap_out) {
                // the unitig whose text holds a place: the first u with ends[u] > g
                const uint64_t ua = (uint64_t)(std::upper_bound(unitig_ends, unitig_ends + n_unitigs, (int64_t)ga) - unitig_ends);
                const uint64_t ub = (uint64_t)(std::upper_bound(unitig_ends, unitig_ends + n_unitigs, (int64_t)gb) - unitig_ends);
                links_out[n_kept] = fin_link{(uint32_t)ua, ga - (uint32_t)(ua ? unitig_ends[ua - 1] : 0), (uint32_t)ub, gb - (uint32_t)(ub ? unitig_ends[ub - 1] : 0),
                                             (uint64_t)(j - i)};
            }
            n_kept++;
        }
        i = j;
    }
    *n_links = n_kept;
    if (counters_out) { counters_out[0] = keys.size(); counters_out[1] = n_distinct; counters_out[2] = n_kept; counters_out[3] = n_self; }
    if (links_out && n_kept > cap_out) return FIN_ELIMIT;
    return FIN_OK;
}
