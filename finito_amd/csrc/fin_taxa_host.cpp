// fin_taxa_host.cpp -- the host twins of fin_taxa.hip (include/finito_amd.h: fin_unitig_lca_labels, fin_taxa_clade_reads), and the one host
// statement of Kraken's rule for a read (fin_taxa_call), which fin_records_read_taxa of fin_records_host.cpp applies to every read.  Plain C++17 with OpenMP: no
// HIP header, no device call (tools/asan_taxa.cpp).  Everything here follows the definitions word for word and makes no use of what the kernels know -- that
// score and clade need only the read's own taxa, that lifting can skip -- so the two can be held against each other.
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

#include "../../include/finito_amd.h"
#include "fin_host.h"
#include "fin_taxa.h"

static_assert(sizeof(fin_read_taxon) == 16, "a read taxon is 16 bytes");

uint64_t fin_taxa_first_bad_parent(const uint32_t* parent, uint64_t n_taxa) {
    if (n_taxa && parent[0] != 0u) return 0;
    for (uint64_t t = 1; t < n_taxa; t++) if ((uint64_t)parent[t] >= t) return t;
    return n_taxa;
}

fin_read_taxon fin_taxa_call(std::vector<std::pair<uint32_t, uint32_t>>& votes, const uint32_t* parent, uint64_t nk, uint32_t min_found, uint32_t confidence_permille) {
    // H with c: the votes sorted and put together
    std::sort(votes.begin(), votes.end());
    size_t n = 0;
    for (size_t i = 0; i < votes.size(); i++) {
        if (n && votes[n - 1].first == votes[i].first) votes[n - 1].second += votes[i].second;
        else votes[n++] = votes[i];
    }
    votes.resize(n);
    if (n == 0) return fin_read_taxon{FIN_NO_LABEL, 0, 0, 0};
    uint64_t n_labelled = 0;
    for (const auto& v : votes) n_labelled += v.second;
    // S and the LCA of the taxa at S
    uint64_t S = 0;
    uint32_t call = FIN_NO_LABEL;
    for (const auto& t : votes) {
        uint64_t score = 0;
        for (const auto& a : votes) if (fin_lca(parent, a.first, t.first) == a.first) score += a.second;
        if (score > S) { S = score; call = t.first; }
        else if (score == S) call = fin_lca(parent, call, t.first);
    }
    // lifting, a level at a time
    const uint64_t need = min_found > 1u ? min_found : 1u;
    for (;;) {
        uint64_t clade = 0;
        for (const auto& x : votes) if (fin_lca(parent, call, x.first) == call) clade += x.second;
        if (!(1000ull * clade < (uint64_t)confidence_permille * nk || clade < need)) return fin_read_taxon{call, (uint32_t)S, (uint32_t)clade, (uint32_t)n_labelled};
        if (call == 0u) return fin_read_taxon{FIN_NO_LABEL, (uint32_t)S, (uint32_t)n_labelled, (uint32_t)n_labelled};
        call = parent[call];
    }
}

int fin_unitig_lca_labels(const uint64_t* bits, uint64_t n_unitigs, uint32_t n_colors, const uint32_t* parent, uint64_t n_taxa, const uint32_t* color_taxon,
                          uint32_t* out, int n_threads) {
    if (n_colors == 0 || n_colors > FIN_MAX_COLORS) return FIN_ELIMIT;
    if (!parent || !color_taxon || n_taxa == 0 || n_taxa > 0x80000000ull || (n_unitigs && (!bits || !out))) return FIN_EINVAL;
    if (fin_taxa_first_bad_parent(parent, n_taxa) != n_taxa) return FIN_EINVAL;
    for (uint32_t c = 0; c < n_colors; c++) if ((uint64_t)color_taxon[c] >= n_taxa) return FIN_EINVAL;
    const uint32_t W = (n_colors + 63u) / 64u;
    if (colors_first_stray(bits, n_unitigs, n_colors, W) != n_unitigs) return FIN_EINVAL;
    const int T = n_threads > 0 ? n_threads : fin_host_threads();
#pragma omp parallel for num_threads(T) schedule(static)
    for (uint64_t u = 0; u < n_unitigs; u++) {
        uint32_t acc = FIN_NO_LABEL;
        for (uint32_t c = 0; c < n_colors; c++)
            if ((bits[u * W + (c >> 6)] >> (c & 63u)) & 1ull) acc = fin_lca(parent, acc, color_taxon[c]);
        out[u] = acc;
    }
    return FIN_OK;
}

int fin_taxa_clade_reads(const uint64_t* direct, const uint32_t* parent, uint64_t n_taxa, uint64_t* clade_out) {
    if (!direct || !parent || !clade_out || n_taxa == 0 || n_taxa > 0x80000000ull) return FIN_EINVAL;
    if (fin_taxa_first_bad_parent(parent, n_taxa) != n_taxa) return FIN_EINVAL;
    for (uint64_t t = 0; t < n_taxa; t++) clade_out[t] = direct[t];
    for (uint64_t t = n_taxa - 1; t >= 1; t--) clade_out[parent[t]] += clade_out[t];   // (children come after their parents)
    return FIN_OK;
}
