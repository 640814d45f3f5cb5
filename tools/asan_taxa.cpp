// The host twins of the taxonomic classification (finito_amd/csrc/fin_taxa_host.cpp and fin_records_read_taxa of fin_records_host.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program: no Python, no device, no HIP.  From the repository root:
//   g++ -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=c++17 -fopenmp -o /tmp/asan_taxa tools/asan_taxa.cpp \
//       finito_amd/csrc/fin_taxa_host.cpp finito_amd/csrc/fin_records_host.cpp
//   /tmp/asan_taxa
// Trees of one node, a chain of 300, a star and a random one; colour rows that are empty, full and the last bit of the last word alone at 1, 64, 65, 130 and
// 4096 colours and 0, 1 and 257 unitigs; records of kind 0, 1 and 2 with reads of 0, 1, 64, 65 and 129 slots and up to 130 distinct taxa; counts up to 2^40;
// buffers of exactly the size the header asks for, with one thread and with three; every refusal.  The expectations are worked out here, by walking root paths.
// It prints "ok" and exits 0 when the calls gave what they must and the sanitizers reported nothing.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "../include/finito_amd.h"

#define MUST(x) do { if (!(x)) { fprintf(stderr, "failed: %s (line %d, tree %d, threads = %d)\n", #x, __LINE__, tree, threads); return 1; } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd64() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static uint32_t rnd(uint32_t n) { return (uint32_t)(rnd64() % n); }

static std::vector<uint32_t> make_tree(int tree) {
    const uint32_t n = tree == 0 ? 1u : tree == 1 ? 300u : tree == 2 ? 140u : 200u;
    std::vector<uint32_t> p(n, 0);
    for (uint32_t t = 1; t < n; t++) p[t] = tree == 1 ? t - 1 : tree == 2 ? 0u : t - 1 - rnd(std::min(t, 5u));
    return p;
}
static std::set<uint32_t> path(const std::vector<uint32_t>& p, uint32_t t) {
    std::set<uint32_t> s{t};
    while (t) { t = p[t]; s.insert(t); }
    return s;
}
static uint32_t lca_all(const std::vector<uint32_t>& p, const std::vector<uint32_t>& ts) {
    if (ts.empty()) return FIN_NO_LABEL;
    std::set<uint32_t> common = path(p, ts[0]);
    for (uint32_t t : ts) { const std::set<uint32_t> q = path(p, t); for (auto it = common.begin(); it != common.end();) it = q.count(*it) ? std::next(it) : common.erase(it); }
    return *common.rbegin();
}
static fin_read_taxon call(const std::vector<uint32_t>& p, const std::map<uint32_t, uint64_t>& c, uint64_t nk, uint32_t min_found, uint32_t conf) {
    if (c.empty()) return fin_read_taxon{FIN_NO_LABEL, 0, 0, 0};
    uint64_t S = 0, n_lab = 0;
    std::map<uint32_t, uint64_t> score;
    for (auto& t : c) { n_lab += t.second; const auto q = path(p, t.first); for (auto& a : c) if (q.count(a.first)) score[t.first] += a.second; S = std::max(S, score[t.first]); }
    std::vector<uint32_t> best;
    for (auto& t : c) if (score[t.first] == S) best.push_back(t.first);
    uint32_t at = lca_all(p, best);
    for (;;) {
        uint64_t clade = 0;
        for (auto& x : c) if (path(p, x.first).count(at)) clade += x.second;
        if (1000 * clade >= (uint64_t)conf * nk && clade >= std::max(min_found, 1u)) return fin_read_taxon{at, (uint32_t)S, (uint32_t)clade, (uint32_t)n_lab};
        if (at == 0) return fin_read_taxon{FIN_NO_LABEL, (uint32_t)S, (uint32_t)n_lab, (uint32_t)n_lab};
        at = p[at];
    }
}

static int run(int tree, int threads) {
    const std::vector<uint32_t> parent = make_tree(tree);
    const uint64_t n_taxa = parent.size();
    // ---- labels from colours
    for (uint32_t n_colors : {1u, 64u, 65u, 130u, 4096u})
        for (uint64_t n : {0ull, 1ull, 257ull}) {
            const uint32_t W = (n_colors + 63u) / 64u;
            std::vector<uint64_t> bits(n * W, 0);
            std::vector<uint32_t> ct(n_colors), got(n, 77), want(n);
            for (auto& t : ct) t = rnd((uint32_t)n_taxa);
            for (uint64_t u = 0; u < n; u++) {
                if (u == 1) for (uint32_t c = 0; c < n_colors; c++) bits[u * W + c / 64] |= 1ull << (c & 63);
                else if (u == 2) bits[u * W + (n_colors - 1) / 64] |= 1ull << ((n_colors - 1) & 63);
                else if (u >= 3) for (uint32_t q = rnd(6); q > 0; q--) { const uint32_t c = rnd(n_colors); bits[u * W + c / 64] |= 1ull << (c & 63); }
                std::vector<uint32_t> ts;
                for (uint32_t c = 0; c < n_colors; c++) if ((bits[u * W + c / 64] >> (c & 63)) & 1) ts.push_back(ct[c]);
                want[u] = lca_all(parent, ts);
            }
            MUST(fin_unitig_lca_labels(n ? bits.data() : nullptr, n, n_colors, parent.data(), n_taxa, ct.data(), n ? got.data() : nullptr, threads) == FIN_OK);
            MUST(got == want);
            ct[n_colors - 1] = (uint32_t)n_taxa;   // a colour's taxon outside the tree
            MUST(fin_unitig_lca_labels(bits.data(), n, n_colors, parent.data(), n_taxa, ct.data(), got.data(), threads) == FIN_EINVAL);
            MUST(fin_unitig_lca_labels(bits.data(), n, 0, parent.data(), n_taxa, ct.data(), got.data(), threads) == FIN_ELIMIT);
            MUST(fin_unitig_lca_labels(bits.data(), n, n_colors, nullptr, n_taxa, ct.data(), got.data(), threads) == FIN_EINVAL);
            MUST(got == want);   // (a refusal writes nothing)
        }
    // ---- read taxa from records + stream
    const int k = 31;
    const uint32_t n_unitigs = 150;
    std::vector<uint32_t> labels(n_unitigs);
    for (uint32_t u = 0; u < n_unitigs; u++) labels[u] = u % 13 == 5 ? FIN_NO_LABEL : (uint32_t)(u % n_taxa);
    std::vector<fin_read_record> recs;
    std::vector<int32_t> stream;
    std::vector<fin_read_taxon> want;
    const uint32_t rules[4][2] = {{1, 0}, {0, 400}, {3, 1000}, {200, 0}};
    for (int rule = 0; rule < 4; rule++) {
        recs.clear(); stream.clear(); want.clear();
        for (uint32_t rep = 0; rep < 400; rep++) {
            std::map<uint32_t, uint64_t> c;
            const uint32_t what = rep % 4;
            if (what == 0) {          // kind 1: one unitig, one position
                const uint32_t u = rnd(n_unitigs), nk = 40 + rnd(60), E = 35 + rnd(20);
                recs.push_back(fin_read_record{u, rnd(50), 1u | ((rep & 4u) << 6) | (1u << 16), nk, E, 0});
                const uint32_t lo = E - 30, hi = std::min(E, nk - 1), found = nk - (hi + 1 - lo);
                if (labels[u] != FIN_NO_LABEL && found) c[labels[u]] = found;
                want.push_back(call(parent, c, nk, rules[rule][0], rules[rule][1]));
            } else if (what == 1) {   // kind 2
                recs.push_back(fin_read_record{0, 0, 2u << 16, rep % 5, 0, 0});
                want.push_back(fin_read_taxon{FIN_NO_LABEL, 0, 0, 0});
            } else {                  // kind 0: 0, 1, 64, 65 or 129 slots over up to 130 unitigs
                const uint32_t nks[5] = {0, 1, 64, 65, 129}, nk = nks[rep % 5], spread = 1 + rnd(130);
                for (uint32_t i = 0; i < nk; i++) {
                    if (rnd(5) == 0) { stream.push_back(-1); stream.push_back(-1); continue; }
                    const uint32_t u = rnd(spread);
                    stream.push_back((int32_t)u); stream.push_back((int32_t)(7 * i));
                    if (labels[u] != FIN_NO_LABEL) c[labels[u]]++;
                }
                recs.push_back(fin_read_record{0, 0, 0, nk, 0, 0});
                want.push_back(call(parent, c, nk, rules[rule][0], rules[rule][1]));
            }
        }
        const uint64_t n = recs.size(), ns = stream.size() / 2;
        std::vector<fin_read_taxon> got(n);
        MUST(fin_records_read_taxa(recs.data(), n, stream.data(), ns, k, labels.data(), n_unitigs, parent.data(), n_taxa, rules[rule][0], rules[rule][1], got.data(), threads) == FIN_OK);
        MUST(memcmp(got.data(), want.data(), n * sizeof(fin_read_taxon)) == 0);
        MUST(fin_records_read_taxa(recs.data(), n, stream.data(), ns - 1, k, labels.data(), n_unitigs, parent.data(), n_taxa, 1, 0, got.data(), threads) == FIN_EINVAL);
        MUST(fin_records_read_taxa(recs.data(), n, stream.data(), ns, k, labels.data(), n_unitigs, parent.data(), n_taxa, 1, 1001, got.data(), threads) == FIN_EINVAL);
        MUST(fin_records_read_taxa(recs.data(), n, stream.data(), ns, k, labels.data(), 10, parent.data(), n_taxa, 1, 0, got.data(), threads) == FIN_EINVAL);   // a unitig outside
    }
    // ---- the roll-up, and what it refuses
    std::vector<uint64_t> direct(n_taxa + 1), clade(n_taxa), wantc(n_taxa, 0);
    for (auto& d : direct) d = rnd(3) ? 0 : rnd64() % (1ull << 40);
    for (uint64_t t = 0; t < n_taxa; t++) for (uint32_t x : path(parent, (uint32_t)t)) wantc[x] += direct[t];
    MUST(fin_taxa_clade_reads(direct.data(), parent.data(), n_taxa, clade.data()) == FIN_OK);
    MUST(clade == wantc);
    MUST(fin_taxa_clade_reads(direct.data(), parent.data(), 0, clade.data()) == FIN_EINVAL);
    if (n_taxa > 2) {
        std::vector<uint32_t> bad = parent;
        bad[2] = 2;
        MUST(fin_taxa_clade_reads(direct.data(), bad.data(), n_taxa, clade.data()) == FIN_EINVAL);
        bad = parent; bad[0] = 1;
        MUST(fin_taxa_clade_reads(direct.data(), bad.data(), n_taxa, clade.data()) == FIN_EINVAL);
    }
    return 0;
}

int main() {
    for (int tree = 0; tree < 4; tree++)
        for (int threads : {1, 3})
            if (run(tree, threads)) return 1;
    printf("ok\n");
    return 0;
}
