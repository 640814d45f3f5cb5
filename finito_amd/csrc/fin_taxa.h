// fin_taxa.h -- the TAXONOMY's two walks, for the device and the host alike (include/finito_amd.h: fin_taxonomy).  parent[n_taxa]: taxon 0 is
// the root, parent[0] == 0, and parent[t] < t for every t >= 1 -- so a walk upward only ever falls, ends at 0, and needs no depth array.  fin_taxa.hip and the
// host twins (fin_taxa_host.cpp, fin_records_host.cpp) take both walks from here.
#pragma once
#include "fin_rec_walk.h"   // (FIN_HD)

#define FIN_TAX_NONE 0xFFFFFFFFu   // FIN_NO_LABEL: "no taxon", the identity of fin_lca

// the lowest common ancestor; FIN_TAX_NONE on either side gives the other
FIN_HD uint32_t fin_lca(const uint32_t* parent, uint32_t a, uint32_t b) {
    if (a == FIN_TAX_NONE) return b;
    if (b == FIN_TAX_NONE) return a;
    while (a != b) { if (a > b) a = parent[a]; else b = parent[b]; }
    return a;
}
// a is an ancestor of t, or t itself (neither is FIN_TAX_NONE): lca(a, t) == a, without walking a
FIN_HD bool fin_tax_covers(const uint32_t* parent, uint32_t a, uint32_t t) {
    while (t > a) t = parent[t];
    return t == a;
}

#if !defined(__HIPCC__)
#include <utility>
#include <vector>

#include "../../include/finito_amd.h"
// the first taxon that breaks the numbering, or n_taxa
uint64_t fin_taxa_first_bad_parent(const uint32_t* parent, uint64_t n_taxa);
// Kraken's rule for one read (include/finito_amd.h states it): votes = (taxon, slots) in any order, a taxon may repeat; nk = the read's output slots
fin_read_taxon fin_taxa_call(std::vector<std::pair<uint32_t, uint32_t>>& votes, const uint32_t* parent, uint64_t nk, uint32_t min_found, uint32_t confidence_permille);
#endif
