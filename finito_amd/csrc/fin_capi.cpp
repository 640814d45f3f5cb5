// fin_capi.cpp -- implementation of the C ABI declared in include/finito_amd.h.
// Host orchestration only: index lifetime, HBM replica, batches, launches.  No CPU search path exists here:
// without a HIP device every search entry point fails with FIN_ENODEV.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/finito_amd.h"
#include "fin_index.hpp"
#include "fin_bootrng.h"
#include "fin_host.h"
#include "fin_kernels.h"
#include "fin_taxa.h"

static void set_err(char* err, size_t errlen, const std::string& msg) {
    if (err && errlen) { snprintf(err, errlen, "%s", msg.c_str()); }
}
#define HIPCHK(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            set_err(err, errlen, std::string(#call) + ": " + hipGetErrorString(e_));                   \
            return FIN_ENODEV;                                                                         \
        }                                                                                              \
    } while (0)

// ---- page-locked staging for callers that hand over pageable buffers ---------------------------------------------------
// A DMA engine cannot read or write pageable memory; the runtime then stages such copies itself, single-threaded.  The pipeline
// below stages through its own page-locked buffers instead: every worker thread copies its sub-batch in and out with the CPU
// while the other workers' sub-batches are on the GPU or on the link.  Buffers are kept in a small process-wide pool.
namespace {
struct StagePool {
    std::mutex mu;
    std::vector<std::pair<void*, size_t>> free_list;
    size_t held = 0;
    void* get(size_t bytes, size_t* cap) {
        {
            std::lock_guard<std::mutex> g(mu);
            size_t best = free_list.size();
            for (size_t i = 0; i < free_list.size(); i++)
                if (free_list[i].second >= bytes && (best == free_list.size() || free_list[i].second < free_list[best].second)) best = i;
            if (best != free_list.size()) {
                void* p = free_list[best].first; *cap = free_list[best].second;
                held -= *cap; free_list.erase(free_list.begin() + (long)best);
                return p;
            }
        }
        void* p = nullptr;
        const size_t want = bytes + bytes / 8 + 4096;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) return nullptr;
        *cap = want;
        return p;
    }
    void put(void* p, size_t cap) {
        if (!p) return;
        {
            std::lock_guard<std::mutex> g(mu);
            if (free_list.size() < 8 && held + cap <= (4ull << 30)) { free_list.push_back({p, cap}); held += cap; return; }
        }
        (void)hipHostFree(p);
    }
    void release_all() {
        std::lock_guard<std::mutex> g(mu);
        for (auto& f : free_list) (void)hipHostFree(f.first);
        free_list.clear(); held = 0;
    }
};
StagePool g_stage;
bool is_page_locked(const void* p) {
    if (!p) return true;
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}
}  // namespace

extern "C" {

const char* fin_version(void) { return "finito-amd 0.1 (gfx950)"; }

// ---- options: process-wide defaults (fin_set_option) and per-index overrides (fin_index_set_option) -------------------------------
// A handle that has its own value of an option uses it, every other handle follows the process-wide value.  The per-handle form is the
// one to use when handles are shared between threads: it touches nothing but its index.
enum : int { O_lds_deque_limit, O_kernel, O_probe_prepass, O_ptab_t, O_jtab_t, O_write_gaps, O_overlap_prefill, O_filt_f, O_seed_anchors, O_kmer_table,
              O_defer_strand, O_fast_path, O_cbf_m, O_lean_tables, O_text_anchors, O_epoch_budget_mult, O_epoch_budget_add, O_max_batch_kmers, O_pipeline_kmers, O_pipeline_depth, O_stage_pageable, O_debug_ovf_cap, O_debug_pp_seg, O_lean_walk, O_fused_ingest, O_pp_park, O_debug_pp_park_cap, O_pp_wide_out, O_hits_combine, O_cover_probe, O_debug_depth_tile, O_ec_tag_bits, O_ec_combine, O_ab_chunk, O_assign_rpb, O_colcov_chunk, O_colsim_chunk, O_colorsets_tag_bits, O_depthhist_unitigs, O_refpaths_tile, O_COUNT };
static_assert(O_COUNT <= FIN_N_OPTIONS, "fin_index::opt_val has room for every option");
struct OptDef { const char* name; int64_t def, lo, hi; };
static const OptDef OPTS[O_COUNT] = {
    {"lds_deque_limit", 16, 1, 16},
    {"kernel", 4, 0, 4},                 // (1 is not a kernel: rejected below)
    {"probe_prepass", 1, 0, 1},          // kernel 3: probe all strands in a separate light kernel first
    {"ptab_t", -1, -1, 15},              // prefix table depth for replicas uploaded from now on: -1 = by index size, 0 = none
    {"jtab_t", -1, -1, 14},              // jump table depth, likewise
    {"write_gaps", 1, 0, 1},             // kernel 4 with seeds: the output is not prefilled, the walk kernel writes absent slots with the pairs
    {"overlap_prefill", 1, 0, 1},        // kernel 4: output prefill on a side stream beside ingest and pre-pass
    {"filt_f", -1, -1, 16},              // depth of the pre-pass's absence filter (-1: by index size, 0: none)
    {"seed_anchors", 1, 0, 1},           // anchor table built at upload, first anchors of a strand found through it (kernel 4)
    {"kmer_table", 1, 0, 1},             // k <= 31: hash table text k-mer -> SBWT node, built with the anchor table, asked instead of whole-k-mer look-ups
    {"defer_strand", 1, 0, 1},           // kernel 4: a read's second strand only where the first left slots open (indexes without reverse-complement pairs and unsafe places)
    {"fast_path", 1, 0, 2},              // kernel 4: the pair pre-pass finishes the reads that lie in one unitig with a few substitutions by itself (fin_prepass.hip); 1 (default) = for k <= 63; 2 = for every k (measured at k = 127: it finishes 55 % of the reads and the step is 11 % slower -- the walk kernel asks the k-mer table above 63 too since round 5, which is what made such a step fast)
    {"cbf_m", -1, -1, 32},               // string length of the two string filters built at upload (-1: min(k, 20), less for k < 29; 0: none -- then no lean tables either)
    {"lean_tables", 2, 0, 3},            // at upload: no prefix table and no anchor table -- the compact k-mer table, the two string filters and the jump table only: probes ask the directional string filter, a string that occurs is followed by a look-up of the whole k-mer.  2 (default since round 5) = for k <= 63: 21 bytes per indexed base at 250 Mbp for any such k; 3 = at every k <= 255 (the walk kernel asks the k-mer table above 63 too: 21 instead of 70 bytes per base at k = 127 -- and a step of 17.0 instead of 10.3 ms: without seeds by node every anchor is a whole-k-mer look-up of ceil(k/32) + 5 epochs); 1 = k <= 31 only (round 4's default: k = 63 then keeps round 3's tables, 68 bytes per base, 6 % faster on iid reads and 32 % slower on a repeat-rich genome); 0 = round 3's tables
    {"text_anchors", 1, 0, 1},           // kernels 3 / 4 re-anchor behind sequencing errors by text comparison, at places the upload found safe
    {"epoch_budget_mult", 64, 0, 64},    // epoch budget of a read: mult * length + add (debug: shrink to force the overflow path)
    {"epoch_budget_add", 4096, 1, 1 << 20},
    {"max_batch_kmers", 1ll << 30, 1, 1ll << 31},
    {"pipeline_kmers", 1ll << 26, 1, 1ll << 31},   // sub-batch size of fin_search_batch's copy/compute pipeline
    {"pipeline_depth", 3, 1, 8},                   // sub-batches in flight per device
    {"stage_pageable", 1, 0, 1},                   // stage pageable caller buffers through page-locked memory inside the pipeline
    {"debug_ovf_cap", 0, 0, 1ll << 31},            // tests: capacity of the overflow list as the kernels see it (0: what the batch allocated)
    {"debug_pp_seg", 0, 0, 1024},                  // tests: reads per block of the pair pre-pass (0: by batch size; else a multiple of 256 up to 1024)
    {"lean_walk", 1, 0, 1},                        // kernel 4, lean tables: the walk kernel's lean instantiations (no prefix-table states: fewer registers); k <= 31: two k-mer-table look-ups per epoch in a run of absent k-mers (round 5)
    {"fused_ingest", 1, 0, 1},                     // kernel 4 with the pre-pass's fast path: no pack kernel -- the fast pre-pass packs the ASCII reads itself and writes the chunks of the reads it does not finish (batches whose reads are all at most FIN_FAST_CHUNKS * 32 bases long); 0 = the pack kernel first (round 5)
    {"pp_park", 1, 0, 1},                          // with the fused ingest: the reads of list A (both first looks failed) stay in LDS for phases 2 and 3 of the fast pre-pass, and only those they do not finish are written out; 0 = every read phase 1 does not finish is written out and read back (round 6)
    {"debug_pp_park_cap", -1, -1, 1024},           // tests: at most this many parked reads per pre-pass block (-1: as many as the LDS budget holds)
    {"pp_wide_out", 1, 0, 1},                      // the fast pre-pass's write-out of the reads it finishes: 1 = from a gap mask the read's own lane makes once, two slots and one 16-byte store per lane (round 13); 0 = slot by slot, every lane comparing its slot with the read's disagreeing positions, 8 bytes per lane
    {"hits_combine", 4, 0, 64},                    // fin_batch_add_hits: what a wave sums before an add goes to memory (fin_hits.hip) -- rounds in which the record lanes of one unitig merge, and the run held back between rows of pairs; 0 = every record lane and every run of a row adds by itself
    {"cover_probe", 0, 0, 1},                      // fin_batch_add_cover: 1 = a lane loads the bitmap word first and skips the atomic OR when every bit it would set is set already (exact: bits are only ever set between resets, fin_cover.hip); 0 = always OR.  Measured (profiles/r09/cover.md): 1 wins behind text-mode-2 steps once the bitmap fills (0.83 against 1.14 ms on chr1), 0 behind default steps (4.0 against 5.0 ms) and summed over both
    {"debug_depth_tile", 0, 0, 4096},              // tests: fin_depth_download's prefix sum in tiles of this many elements and chunks of 64 tiles (0: tiles of 4096 elements, chunks of 4096 tiles)
    {"ec_tag_bits", 63, 1, 63},                    // fin_eqclasses: bits of a row's tag in the table (fin_eqclasses.hip); tests narrow it so that distinct rows share tags and go through the serial pass.  Read by the first add after the accumulator's creation or reset and kept until the next reset: a table's tags are made one way
    {"ec_combine", 1, 0, 1},                       // fin_eqclasses' count pass: 1 = a wave's adds combined over its distinct slots, one atomic each; 0 = one atomic per row (tools/ab_eqclasses.py measures both)
    {"ab_chunk", 0, 0, 1ll << 26},                 // fin_eqclasses_abundance's column pass: classes per chunk, rounded up to a multiple of 64 (fin_abundance.hip); 0 = auto: 256, more once that would make over 1024 chunks (which also bounds what a value can ask for).  The order of the column sums is a function of it, so two estimates compare bit for bit only under one value; tests set 64 so that small cases cross chunk seams
    {"assign_rpb", 0, 0, 1ll << 26},               // fin_assign_rows: rows per block of fin_assign_rows_kernel (fin_assign.hip); 0 = auto: 1024, more once that would make over 2048 blocks; never so few that there would be over 2^20 blocks.  The results do not depend on it; tests set 64 so that small cases cross block seams
    {"colcov_chunk", 0, 0, 1ll << 26},             // fin_colors_coverage: unitigs per chunk of fin_colcov_column_kernel (fin_colcov.hip), rounded up to a multiple of 64; 0 = auto: 1024, more once that would make over 8192 waves; never so few that there would be over 2^20 chunks.  The results do not depend on it; tests set 64 so that small cases cross chunk seams
    {"colsim_chunk", 0, 0, 1ll << 26},             // fin_colors_shared: unitigs per chunk of fin_colsim_tile_kernel (fin_colsim.hip), rounded up to a multiple of 64; 0 = auto: 4096, more once that would make over 16384 waves; never so few that tiles x chunks would pass 2^30 blocks.  The results do not depend on it; tests set 64 so that small cases cross chunk seams
    {"colorsets_tag_bits", 31, 1, 31},             // fin_colors_compact: bits of a row's tag in the dedup table (fin_colorsets.hip); the home slot is a function of the tag, so tests narrow it to force distinct rows under one tag and long probe chains.  The results do not depend on it
    {"depthhist_unitigs", 0, 0, 1ll << 26},        // fin_colors_depth_histogram: unitigs per sub-range of a staged chunk, each binned into a table uint32[unitigs][n_bins] and projected (fin_depthhist.hip); 0 = auto: what a table of 64 MB holds, at least 64.  A value is cut to that budget too.  The results do not depend on it; tests set 16 so that small cases cross sub-range seams
    {"refpaths_tile", 0, 0, 1ll << 26},            // fin_refpaths_depth: slots of a segment per tile, a wave's work in fin_rp_depth_kernel (fin_refpaths.hip), rounded up to a multiple of 64; 0 = auto: 4096.  The results do not depend on it; tests set 64 so that small segments cross tile seams
};
static std::atomic<int64_t> g_opt[O_COUNT];
static const bool g_opt_init = [] { for (int i = 0; i < O_COUNT; i++) g_opt[i].store(OPTS[i].def); return true; }();
static inline int64_t optv(const fin_index* x, int id) { return x && x->opt_set[id].load(std::memory_order_acquire) ? x->opt_val[id].load(std::memory_order_relaxed) : g_opt[id].load(std::memory_order_relaxed); }
static int opt_find(const char* name, int64_t value) {
    if (!name) return -1;
    for (int i = 0; i < O_COUNT; i++)
        if (!strcmp(name, OPTS[i].name)) return (value < OPTS[i].lo || value > OPTS[i].hi || (i == O_kernel && value == 1)) ? -1 : i;
    return -1;
}

int fin_set_option(const char* name, int64_t value) {
    (void)g_opt_init;
    const int id = opt_find(name, value);
    if (id < 0) return FIN_EINVAL;
    g_opt[id].store(value);
    if (id == O_stage_pageable && !value) g_stage.release_all();
    return FIN_OK;
}

int fin_index_set_option(fin_index* idx, const char* name, int64_t value) {
    if (!idx) return FIN_EINVAL;
    const int id = opt_find(name, value);
    if (id < 0) return FIN_EINVAL;
    idx->opt_val[id].store(value, std::memory_order_relaxed); idx->opt_set[id].store(true, std::memory_order_release);   // (a reader that sees the flag sees the value)
    return FIN_OK;
}

int fin_index_clear_option(fin_index* idx, const char* name) {
    if (!idx || !name) return FIN_EINVAL;
    for (int i = 0; i < O_COUNT; i++) if (!strcmp(name, OPTS[i].name)) { idx->opt_set[i].store(false); return FIN_OK; }
    return FIN_EINVAL;
}

int fin_index_build(const char* unitig_bases, const uint64_t* unitig_offsets, uint64_t n_unitigs, int k, int n_threads,
                    fin_index** out, char* err, size_t errlen) {
    if (!unitig_bases || !unitig_offsets || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    fin_index* x = new (std::nothrow) fin_index();
    if (!x) { set_err(err, errlen, "out of memory"); return FIN_ENOMEM; }
    std::string msg;
    int rc;
    try {
        rc = fin_build_index(unitig_bases, unitig_offsets, n_unitigs, k, n_threads > 0 ? n_threads : fin_host_threads(), *x, msg);
    } catch (const std::bad_alloc&) { rc = FIN_ENOMEM; msg = "out of memory while building the index"; }
    if (rc != 0) { delete x; set_err(err, errlen, msg); return rc; }
    *out = x;
    return FIN_OK;
}

int fin_index_build_device(const char* unitig_bases, const uint64_t* unitig_offsets, uint64_t n_unitigs, int k, int device,
                           fin_index** out, double* phase_ms, char* err, size_t errlen) {
    if (!unitig_bases || !unitig_offsets || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_err(err, errlen, "no HIP device available (fin_index_build is the host builder)"); return FIN_ENODEV; }
    if (device < 0 || device >= ndev) { set_err(err, errlen, "device ordinal out of range"); return FIN_EINVAL; }
    fin_index* x = new (std::nothrow) fin_index();
    if (!x) { set_err(err, errlen, "out of memory"); return FIN_ENOMEM; }
    std::string msg;
    int rc;
    try { rc = fin_build_index_gpu(unitig_bases, unitig_offsets, n_unitigs, k, device, *x, msg, phase_ms); }
    catch (const std::bad_alloc&) { rc = FIN_ENOMEM; msg = "out of memory while building the index"; }
    if (rc != 0) { delete x; set_err(err, errlen, msg); return rc == -3 ? FIN_ENODEV : rc; }
    *out = x;
    return FIN_OK;
}

static bool file_exists(const std::string& p) { FILE* f = fopen(p.c_str(), "rb"); if (f) fclose(f); return f != nullptr; }

// <prefix>.finparts, the manifest of a partitioned index (fin_pindex_save writes it, below): what it says, for the loader and for whoever saves over it
struct PartsManifest {
    int k = 0;
    unsigned long long n_unitigs = 0; long long shared_kmers = -1;
    std::vector<uint64_t> first_unitig;   // per part
    std::vector<size_t> n_part_unitigs;   // per part
    size_t parts() const { return n_part_unitigs.size(); }
};
// -1: no such file; 0: a file that is not a manifest; 1: read
static int read_parts_manifest(const std::string& pre, PartsManifest& m) {
    FILE* f = fopen((pre + ".finparts").c_str(), "r");
    if (!f) return -1;
    int ver = 0; size_t P = 0;
    bool ok = fscanf(f, "finito-parts %d k %d parts %zu unitigs %llu shared_kmers %lld", &ver, &m.k, &P, &m.n_unitigs, &m.shared_kmers) == 5 && ver == 1 && P >= 1 && P < 65536;
    m.first_unitig.assign(ok ? P : 0, 0); m.n_part_unitigs.assign(ok ? P : 0, 0);
    for (size_t p = 0; ok && p < P; p++) {
        size_t pi = 0; unsigned long long fu = 0;
        ok = fscanf(f, " part %zu first_unitig %llu unitigs %zu", &pi, &fu, &m.n_part_unitigs[p]) == 3 && pi == p;
        m.first_unitig[p] = fu;
    }
    fclose(f);
    if (!ok) { m.first_unitig.clear(); m.n_part_unitigs.clear(); }
    return ok ? 1 : 0;
}
// a file that is not there is removed already; one that is there and stays is an error
static int remove_file(const std::string& path, char* err, size_t errlen) {
    if (std::remove(path.c_str()) == 0 || errno == ENOENT) return FIN_OK;
    set_err(err, errlen, "cannot remove " + path + ": " + strerror(errno));
    return FIN_EIO;
}
// part i's container and table of set-wide unitig numbers, for i in [from, to)
static int remove_part_files(const std::string& pre, size_t from, size_t to, char* err, size_t errlen) {
    for (size_t i = from; i < to; i++)
        for (const char* ext : {".finamd", ".gid"})
            if (const int rc = remove_file(pre + ".p" + std::to_string(i) + ext, err, errlen)) return rc;
    return FIN_OK;
}

static int index_save_container(const fin_index* idx, const char* prefix, char* err, size_t errlen) {
    std::string msg;
    int rc = fin_save_index(*idx, prefix, msg);
    if (rc) set_err(err, errlen, msg);
    return rc;
}

// Saving under a prefix REPLACES what was there: loaders take the partitioned index whenever <prefix>.finparts exists (FinimizerIndex::load, search-fmin), so a
// manifest an earlier fin_pindex_save left under this prefix would answer for the index written here.  It goes first (from then on the prefix is this index),
// then the part files it names, if it can be read.
int fin_index_save(const fin_index* idx, const char* prefix, char* err, size_t errlen) {
    if (!idx || !prefix) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int rc = index_save_container(idx, prefix, err, errlen)) return rc;
    const std::string pre(prefix);
    PartsManifest old;
    const int had = read_parts_manifest(pre, old);
    if (had < 0) return FIN_OK;
    if (const int rc = remove_file(pre + ".finparts", err, errlen)) return rc;
    return remove_part_files(pre, 0, old.parts(), err, errlen);
}

int fin_index_load(const char* prefix, fin_index** out, char* err, size_t errlen) {
    if (!prefix || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    fin_index* x = new (std::nothrow) fin_index();
    if (!x) { set_err(err, errlen, "out of memory"); return FIN_ENOMEM; }
    std::string msg;
    int rc;
    try {
        // the container file if there is one, else the reference's own seven files (an index built by the reference's tools)
        const std::string p(prefix);
        if (!file_exists(p + ".finamd") && file_exists(p + ".sbwt")) rc = fin_load_reference_layout(p, *x, msg);
        else rc = fin_load_index(p, *x, msg);
    } catch (const std::bad_alloc&) { rc = FIN_ENOMEM; msg = "out of memory"; }
    if (rc) { delete x; set_err(err, errlen, msg); return rc; }
    *out = x;
    return FIN_OK;
}

int fin_index_load_reference_layout(const char* prefix, fin_index** out, char* err, size_t errlen) {
    if (!prefix || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    fin_index* x = new (std::nothrow) fin_index();
    if (!x) { set_err(err, errlen, "out of memory"); return FIN_ENOMEM; }
    std::string msg;
    int rc;
    try { rc = fin_load_reference_layout(prefix, *x, msg); } catch (const std::bad_alloc&) { rc = FIN_ENOMEM; msg = "out of memory"; }
    if (rc) { delete x; set_err(err, errlen, msg); return rc; }
    *out = x;
    return FIN_OK;
}

int fin_index_save_reference_layout(const fin_index* idx, const char* prefix, char* err, size_t errlen) {
    if (!idx || !prefix) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    std::string msg;
    int rc;
    try { rc = fin_save_reference_layout(*idx, prefix, msg); } catch (const std::bad_alloc&) { rc = FIN_ENOMEM; msg = "out of memory"; }
    if (rc) set_err(err, errlen, msg);
    return rc;
}

int fin_index_save_sbwt(const fin_index* idx, const char* path, char* err, size_t errlen) {
    if (!idx || !path) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    std::string msg;
    int rc;
    try { rc = fin_save_sbwt_file(*idx, path, msg); } catch (const std::bad_alloc&) { rc = FIN_ENOMEM; msg = "out of memory"; }
    if (rc) set_err(err, errlen, msg);
    return rc;
}

int fin_sbwt_file_info(const char* path, int64_t* k, int64_t* n_nodes, int64_t* n_kmers, char* err, size_t errlen) {
    if (!path) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    std::string msg; int64_t a = 0, b = 0, c = 0;
    int rc;
    try { rc = fin_read_sbwt_file(path, true, a, b, c, nullptr, msg); } catch (const std::bad_alloc&) { rc = FIN_ENOMEM; msg = "out of memory"; }
    if (rc) { set_err(err, errlen, msg); return rc; }
    if (k) *k = a;
    if (n_nodes) *n_nodes = b;
    if (n_kmers) *n_kmers = c;
    return FIN_OK;
}

int fin_index_check_against_files(const fin_index* idx, const char* sbwt_path, const char* lcs_path, char* err, size_t errlen) {
    if (!idx) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    std::string msg; int rc = 0;
    try {
        int64_t a, b, c;
        if (sbwt_path && *sbwt_path) rc = fin_read_sbwt_file(sbwt_path, true, a, b, c, idx, msg);
        if (rc == 0 && lcs_path && *lcs_path) rc = fin_check_lcs_file(lcs_path, *idx, msg);
    } catch (const std::bad_alloc&) { rc = FIN_ENOMEM; msg = "out of memory"; }
    if (rc) set_err(err, errlen, msg);
    return rc;
}

static void free_replica(fin_index::Replica& r) {
    if (r.device >= 0) {
        (void)hipSetDevice(r.device);
        (void)hipFree(r.d_blocks); (void)hipFree(r.d_blkinfo); (void)hipFree(r.d_goff); (void)hipFree(r.d_ends); (void)hipFree(r.d_samp); (void)hipFree(r.d_concat); (void)hipFree(r.d_ptab); (void)hipFree(r.d_jtab); (void)hipFree(r.d_pos); (void)hipFree(r.d_filt); (void)hipFree(r.d_lcs8); (void)hipFree(r.d_safe); (void)hipFree(r.d_kt3); (void)hipFree(r.d_ktx); (void)hipFree(r.d_rcwin); (void)hipFree(r.d_cbf); (void)hipFree(r.d_fbf);
        r = fin_index::Replica();
    }
}
static void free_device(fin_index* x) {
    for (auto& r : x->replicas) free_replica(r);
    x->replicas.clear();
}

void fin_batch_free(fin_batch* b);
void fin_index_free(fin_index* idx) {
    if (!idx) return;
    for (auto& pb : idx->batch_pool) fin_batch_free(pb.second);
    idx->batch_pool.clear();
    free_device(idx);
    delete idx;
}

int64_t fin_index_k(const fin_index* x) { return x ? (int64_t)x->k : -1; }
int64_t fin_index_n_nodes(const fin_index* x) { return x ? (int64_t)x->n_nodes : -1; }
int64_t fin_index_n_kmers(const fin_index* x) { return x ? (int64_t)x->n_kmers : -1; }
int64_t fin_index_n_unitigs(const fin_index* x) { return x ? (int64_t)x->n_unitigs : -1; }
int64_t fin_index_n_finimizers(const fin_index* x) { return x ? (int64_t)x->n_fmin : -1; }
int64_t fin_index_total_len(const fin_index* x) { return x ? (int64_t)x->total_len : -1; }
int fin_index_prefix_table_depth(const fin_index* x, int device) {
    if (!x) return -1;
    const fin_index::Replica* r = x->replica_on(device);
    return r ? (int)r->dev.ptab_t : -1;
}

// 1: the number of distinct k-mers equals the number of k-mer positions in the unitigs (every k-mer has exactly one place).  Informative
// only: what the kernels may take from the text is decided per k-mer at upload (fin_index_unsafe_places).
int fin_index_is_disjoint(const fin_index* x) {
    if (!x || !x->n_unitigs) return 0;
    uint64_t places = 0;
    for (uint64_t u = 0; u < x->n_unitigs; u++) {
        const uint64_t len = (uint64_t)x->ends[u + 1] - x->ends[u];
        if (len >= x->k) places += len - x->k + 1;
    }
    return x->n_kmers == places ? 1 : 0;
}

int64_t fin_index_rc_pairs(const fin_index* x, int device) {
    if (!x) return -1;
    const fin_index::Replica* r = x->replica_on(device);
    return r && r->anchors_built && r->n_rc_pairs != ~0ull ? (int64_t)r->n_rc_pairs : -1;
}
int64_t fin_index_unsafe_places(const fin_index* x, int device) {
    if (!x) return -1;
    const fin_index::Replica* r = x->replica_on(device);
    return r && r->anchors_built ? (int64_t)r->n_unsafe : -1;
}
double fin_index_anchor_build_ms(const fin_index* x, int device) {
    const fin_index::Replica* r = x ? x->replica_on(device) : nullptr;
    return r && r->anchors_built ? r->anchors_ms : -1.0;
}

// k-mer places whose k-mer has an unverified answer (the reference reports a place that does not spell it): what the exact side table holds; -1: no replica / no anchor pass
int64_t fin_index_unverified_kmers(const fin_index* x, int device) {
    if (!x) return -1;
    const fin_index::Replica* r = x->replica_on(device);
    return r && r->anchors_built ? (int64_t)r->n_unverified : -1;
}
int64_t fin_index_kmer_table_bytes(const fin_index* x, int device) {
    if (!x) return -1;
    const fin_index::Replica* r = x->replica_on(device);
    return r ? (r->d_kt3 ? (int64_t)(32ull * r->dev.kt3_buckets + (r->d_ktx ? (32ull << r->dev.ktx_log2) : 0)) : 0) : -1;
}

// the device of the handle's first (default) replica, -1: none
int fin_index_first_device(const fin_index* x) { return (x && !x->replicas.empty()) ? x->replicas[0].device : -1; }
// HBM of the replica on `device` beyond the index arrays (fin_index_size_in_bytes): every table, filter and bitmap the upload built
int64_t fin_index_replica_table_bytes(const fin_index* x, int device) {
    if (!x) return -1;
    const fin_index::Replica* r = x->replica_on(device);
    return r ? (int64_t)r->table_bytes : -1;
}
int64_t fin_index_string_filter_bytes(const fin_index* x, int device) {
    if (!x) return -1;
    const fin_index::Replica* r = x->replica_on(device);
    return r ? (r->d_cbf ? (int64_t)(16ull << r->dev.cbf_log2) : 0) : -1;
}

int64_t fin_index_seed_table_bytes(const fin_index* x, int device) {
    if (!x) return -1;
    const fin_index::Replica* r = x->replica_on(device);
    return r ? (r->d_pos ? (int64_t)x->n_nodes * (int64_t)sizeof(FinSeedEntry) : 0) : -1;
}

int fin_index_filter_depth(const fin_index* x, int device) {
    if (!x) return -1;
    const fin_index::Replica* r = x->replica_on(device);
    return r ? (int)r->dev.filt_f : -1;
}

int fin_index_jump_table_depth(const fin_index* x, int device) {
    if (!x) return -1;
    const fin_index::Replica* r = x->replica_on(device);
    return r ? (int)r->dev.jtab_t : -1;
}

int64_t fin_index_size_in_bytes(const fin_index* x) {
    if (!x) return -1;
    return (int64_t)(x->blocks.n * sizeof(FinNodeBlock) + x->blkinfo.size() * sizeof(FinBlockInfo) + 4 * (x->goff.size() + x->ends.size() + x->samp.size() + x->concat.size()));
}

int64_t fin_index_export_size(const fin_index* x, int what) {
    if (!x) return -1;
    const int64_t nw = (int64_t)((x->n_nodes + 63) / 64);
    switch (what) {
        case FIN_X_C: return 32;
        case FIN_X_PLANE_A: case FIN_X_PLANE_A + 1: case FIN_X_PLANE_A + 2: case FIN_X_PLANE_A + 3: return nw * 8;
        case FIN_X_LCS: return (int64_t)x->n_nodes;
        case FIN_X_FMIN: case FIN_X_USTART: return nw * 8;
        case FIN_X_GOFF: return (int64_t)x->n_fmin * 8;
        case FIN_X_ENDS: return (int64_t)x->n_unitigs * 8;
        case FIN_X_CONCAT: return (int64_t)x->total_len;
        default: return -1;
    }
}

int fin_index_export(const fin_index* x, int what, void* out, uint64_t out_bytes, char* err, size_t errlen) {
    int64_t need = fin_index_export_size(x, what);
    if (need < 0 || !out) { set_err(err, errlen, "bad export selector or null buffer"); return FIN_EINVAL; }
    if (out_bytes < (uint64_t)need) { set_err(err, errlen, "export buffer too small"); return FIN_EINVAL; }
    const FinNodeBlock* B = x->blocks.p;
    const uint64_t nb = x->blocks.n;
    switch (what) {
        case FIN_X_C: for (int c = 0; c < 4; c++) ((int64_t*)out)[c] = (int64_t)x->C[c]; break;
        case FIN_X_PLANE_A: case FIN_X_PLANE_A + 1: case FIN_X_PLANE_A + 2: case FIN_X_PLANE_A + 3:
            for (uint64_t b = 0; b < nb; b++) ((uint64_t*)out)[b] = fin_plane(B[b].rec[what - FIN_X_PLANE_A]);
            break;
        case FIN_X_LCS: for (uint64_t i = 0; i < x->n_nodes; i++) ((uint8_t*)out)[i] = (uint8_t)fin_host_lcs(B, x->lcs8_or_null(), (int64_t)i); break;
        case FIN_X_FMIN: for (uint64_t b = 0; b < nb; b++) ((uint64_t*)out)[b] = x->blkinfo[b].fmin_mask_lo | ((uint64_t)x->blkinfo[b].fmin_mask_hi << 32); break;
        case FIN_X_USTART:
            for (uint64_t b = 0; b < nb; b++) {
                uint64_t w = 0;   // from the per-node flags; the builder keeps ustart_mask identical (checked in tests)
                for (int j = 0; j < 64; j++) if (B[b].node[j] & FIN_USTART_BIT) w |= 1ull << j;
                ((uint64_t*)out)[b] = w == (x->blkinfo[b].ustart_mask_lo | ((uint64_t)x->blkinfo[b].ustart_mask_hi << 32)) ? w : ~0ull;
            }
            break;
        case FIN_X_GOFF: for (uint64_t i = 0; i < x->n_fmin; i++) ((int64_t*)out)[i] = (int64_t)x->goff[i]; break;
        case FIN_X_ENDS: for (uint64_t i = 0; i < x->n_unitigs; i++) ((int64_t*)out)[i] = (int64_t)x->ends[i + 1]; break;
        case FIN_X_CONCAT: for (uint64_t i = 0; i < x->total_len; i++) ((uint8_t*)out)[i] = (uint8_t)((x->concat[i >> 4] >> (2 * (i & 15))) & 3u); break;
    }
    return FIN_OK;
}

int fin_index_to_device(fin_index* x, int device, char* err, size_t errlen) {
    if (!x) { set_err(err, errlen, "null index"); return FIN_EINVAL; }
    if (x->replica_on(device)) return FIN_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_err(err, errlen, "no HIP device available (this path has no CPU fallback)"); return FIN_ENODEV; }
    if (device < 0 || device >= ndev) { set_err(err, errlen, "device ordinal out of range"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(device));
    fin_index::Replica r;
    r.device = device;
    auto up = [&](void** d, const void* h, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(d, bytes ? bytes : 4);
        if (e != hipSuccess) return e;
        return bytes ? hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) : hipSuccess;
    };
    hipError_t e;
    if ((e = up(&r.d_blocks, x->blocks.p, x->blocks.n * sizeof(FinNodeBlock))) != hipSuccess ||
        (e = up(&r.d_blkinfo, x->blkinfo.data(), x->blkinfo.size() * sizeof(FinBlockInfo))) != hipSuccess ||
        (e = up(&r.d_goff, x->goff.data(), x->goff.size() * 4)) != hipSuccess ||
        (e = up(&r.d_ends, x->ends.data(), x->ends.size() * 4)) != hipSuccess ||
        (e = up(&r.d_samp, x->samp.data(), x->samp.size() * 4)) != hipSuccess ||
        (e = up(&r.d_concat, x->concat.data(), x->concat.size() * 4)) != hipSuccess) {
        free_replica(r);
        set_err(err, errlen, std::string("uploading the index: ") + hipGetErrorString(e));
        return FIN_ENODEV;
    }
    FinDevIndex& d = r.dev;
    d.blocks = (const FinNodeBlock*)r.d_blocks; d.blkinfo = (const FinBlockInfo*)r.d_blkinfo; d.goff = (const uint32_t*)r.d_goff;
    d.ends = (const uint32_t*)r.d_ends; d.samp = (const uint32_t*)r.d_samp; d.concat = (const uint32_t*)r.d_concat;
    d.n_nodes = (uint32_t)x->n_nodes; d.n_unitigs = (uint32_t)x->n_unitigs; d.total_len = (uint32_t)x->total_len; d.k = x->k;
    d.samp_shift = x->samp_shift; d.n_samp = (uint32_t)x->samp.size();
    for (int c = 0; c < 4; c++) d.C[c] = (uint32_t)x->C[c];
    d.C[4] = (uint32_t)x->n_nodes;
    d.lcs_t0 = x->lcs_t0;
    d.lcs8 = nullptr;
    if (!x->lcs8.empty()) {   // k > 128: the exact LCS array for the plain kernel (the node bytes hold min(LCS, 127))
        if ((e = up(&r.d_lcs8, x->lcs8.data(), x->lcs8.size())) != hipSuccess) {
            free_replica(r); set_err(err, errlen, std::string("uploading the LCS array: ") + hipGetErrorString(e)); return FIN_ENODEV;
        }
        d.lcs8 = (const uint8_t*)r.d_lcs8;
    }
    d.budget_mult = 64; d.budget_add = 4096;
    d.text_anchors = 0; d.defer_ok = 0; d.rcwin = nullptr;   // (set per run: fin_batch_run)
    {   // prefix table for the kernel's probe mode: depth T with 4^T <= 16 * n_nodes (most random T-mers are then already absent --
        // one table line settles the probe -- and T+4 bases almost never occur), at most 15 (8 GiB of the 288) and at most k;
        // filled on the device from the blocks just uploaded
        // (option cbf_m 0 = no string filters: lean tables need the directional one -- round 3's tables are built instead)
        const bool lean_req = optv(x, O_lean_tables) && optv(x, O_cbf_m) != 0 && optv(x, O_ptab_t) < 0 && x->k <= (optv(x, O_lean_tables) >= 3 ? 255u : optv(x, O_lean_tables) >= 2 ? 63u : 31u) && optv(x, O_kmer_table) && optv(x, O_seed_anchors) && optv(x, O_text_anchors) &&
                              x->total_len < FIN_POS_DUMMY && x->n_unitigs < FIN_POS_UNVERIFIED;
        int T = lean_req ? 0 : (int)optv(x, O_ptab_t);
        if (T < 0) { T = 0; while (T < 15 && T < (int)x->k && (1ull << (2 * (T + 1))) <= 16ull * x->n_nodes) T++; }
        if (T > (int)x->k) T = (int)x->k;
        d.ptab_t = 0; d.ptab = nullptr;
        if (T > 0) {
            if ((e = hipMalloc(&r.d_ptab, (sizeof(FinPrefixIval) << (2 * T)) + 16)) != hipSuccess) {
                free_replica(r); set_err(err, errlen, std::string("prefix table: ") + hipGetErrorString(e)); return FIN_ENODEV;
            }
            d.ptab_t = (uint32_t)T; d.ptab = (const FinPrefixIval*)r.d_ptab;
            const int rc = fin_launch_build_ptab(&d, r.d_ptab, T, nullptr);
            if (rc != 0 || (e = hipDeviceSynchronize()) != hipSuccess) {
                free_replica(r); set_err(err, errlen, std::string("prefix table kernel: ") + hipGetErrorString(rc ? (hipError_t)rc : e)); return FIN_ENODEV;
            }
        }
    }
    {   // jump table for (re)started streaming searches: depth J with 4^J <= n_nodes / 3 (nearly every J-base string of the indexed text
        // then occurs at least twice, which is what a jump needs), below k, at most 14
        int J = (int)optv(x, O_jtab_t);
        if (J < 0) { J = 0; while (J < 14 && 3ull * (1ull << (2 * (J + 1))) <= x->n_nodes) J++; }
        if (J >= (int)x->k) J = (int)x->k - 1;
        d.jtab_t = 0; d.jtab = nullptr;
        if (J > 0) {
            if ((e = hipMalloc(&r.d_jtab, (sizeof(FinPrefixIval) << (2 * J)) + 16)) != hipSuccess) {
                free_replica(r); set_err(err, errlen, std::string("jump table: ") + hipGetErrorString(e)); return FIN_ENODEV;
            }
            const int rc = fin_launch_build_ptab(&d, r.d_jtab, J, nullptr);
            if (rc != 0 || (e = hipDeviceSynchronize()) != hipSuccess) {
                free_replica(r); set_err(err, errlen, std::string("jump table kernel: ") + hipGetErrorString(rc ? (hipError_t)rc : e)); return FIN_ENODEV;
            }
            d.jtab_t = (uint32_t)J; d.jtab = (const FinPrefixIval*)r.d_jtab;
        }
    }
    {   // absence filter of the pre-pass.  By default only where its bit set stays in the L2 (4^F bits <= 2 MB: F <= 12) AND is sparse enough
        // to say something (4^F >= the text's length): small indexes.  Measured on the 250 Mbp index (F = 14, 32 MB, Infinity-Cache
        // resident): the pre-pass got SLOWER (5.2 -> 6.4 ms) -- a look-up that misses the L2 costs a request like a prefix-table line
        // does, wherever it is served from, and the filter asks more often than it saves (CHANGELOG.md 5.5).
        int F = (int)optv(x, O_filt_f);
        if (F < 0) { F = 8; while (F < 12 && (1ull << (2 * F)) < x->total_len) F++; if ((1ull << (2 * F)) < x->total_len) F = 0; }
        if (F >= (int)x->k) F = (int)x->k - 1;
        d.filt = nullptr; d.filt_f = 0;
        if (F >= 4) {
            if ((e = hipMalloc(&r.d_filt, ((1ull << (2 * F)) / 32 + 8) * 4)) != hipSuccess) {
                free_replica(r); set_err(err, errlen, std::string("absence filter: ") + hipGetErrorString(e)); return FIN_ENODEV;
            }
            const int rc = fin_launch_build_filter(&d, (uint32_t*)r.d_filt, F, nullptr);
            if (rc != 0 || (e = hipDeviceSynchronize()) != hipSuccess) {
                free_replica(r); set_err(err, errlen, std::string("absence filter kernel: ") + hipGetErrorString(rc ? (hipError_t)rc : e)); return FIN_ENODEV;
            }
            d.filt = (const uint32_t*)r.d_filt; d.filt_f = (uint32_t)F;
        }
    }
    d.pos = nullptr; d.safe = nullptr; d.kt3 = nullptr; d.kt3_buckets = 0; d.ktx = nullptr; d.ktx_log2 = 0;
    const bool up_seeds = optv(x, O_seed_anchors) != 0, up_text = optv(x, O_text_anchors) != 0;
    if ((up_seeds || up_text) && x->total_len < FIN_POS_DUMMY && x->n_unitigs < FIN_POS_UNVERIFIED && x->k < 256) {
        // anchor table (FinDevIndex::pos) and safe-place bitmap (FinDevIndex::safe): the unitig text streamed through the plain search on
        // the device (fin_kernel_b.hip) -- per node the reference's answer for its k-mer, per text position whether the k-mer there is
        // reported there.  16 bytes per node + 1 bit per base; the bitmap is dropped when every place is safe (disjoint unitigs).
        void* d_tmp = nullptr;
        // k-mer table (with the anchor pass): the COMPACT table of round 5 -- 8-byte slots {answer, tag}, four to a 32-byte bucket, 55 % full: room for
        // the text's k-mer positions / 0.55, whatever the text's size (bucket numbers are 32-bit: up to 2^34 slots; the answers are text offsets below 2^32)
        uint32_t kt3_buckets = 0;
        if (optv(x, O_kmer_table) && up_seeds) {   // (any k <= 255 since the walk kernel folds a long k-mer's words into the hash as its chunks arrive, fin_kernel_w.hip W_KF0B)
            uint64_t places = 0;
            for (uint64_t u = 0; u < x->n_unitigs; u++) { const uint64_t len = (uint64_t)x->ends[u + 1] - x->ends[u]; if (len >= x->k) places += len - x->k + 1; }
            const uint64_t nb = (places * 100 / FIN_KT3_LOAD_PCT + FIN_KT3_SLOTS - 1) / FIN_KT3_SLOTS + 16;
            if (nb < 0xFFFFFFF0ull) {
                kt3_buckets = (uint32_t)nb;
                if ((e = hipMalloc(&r.d_kt3, 32ull * kt3_buckets)) != hipSuccess) {
                    free_replica(r); set_err(err, errlen, std::string("k-mer table: ") + hipGetErrorString(e)); return FIN_ENODEV;
                }
            }
        }
        r.lean = optv(x, O_lean_tables) && optv(x, O_cbf_m) != 0 && optv(x, O_ptab_t) < 0 && optv(x, O_text_anchors) && kt3_buckets != 0 && x->k <= (optv(x, O_lean_tables) >= 3 ? 255u : optv(x, O_lean_tables) >= 2 ? 63u : 31u);   // (a k-mer table: the conditions under which no prefix table was built above)
        if ((!r.lean && (e = hipMalloc(&r.d_pos, ((size_t)x->n_nodes + 1) * sizeof(FinSeedEntry))) != hipSuccess) ||
            (e = hipMalloc(&r.d_safe, fin_anchor_safe_words(x->total_len) * 8)) != hipSuccess ||
            (e = hipMalloc(&d_tmp, fin_anchor_tmp_bytes(x->total_len))) != hipSuccess) {
            (void)hipFree(d_tmp); free_replica(r); set_err(err, errlen, std::string("anchor table: ") + hipGetErrorString(e)); return FIN_ENODEV;
        }
        hipEvent_t t0 = nullptr, t1 = nullptr;
        (void)hipEventCreate(&t0); (void)hipEventCreate(&t1);
        (void)hipEventRecord(t0, nullptr);
        uint64_t n_unver = 0;
        int rc = fin_launch_build_anchors(&d, (FinSeedEntry*)r.d_pos, r.d_safe, r.d_kt3, kt3_buckets, d_tmp, &r.n_unsafe, nullptr, &n_unver);
        uint32_t ktx_lg = 0;
        if (rc == 0 && r.d_kt3 && n_unver) {
            // the exact side table of the k-mers whose answer is unverified (FinDevIndex::ktx), from the list the pass left in d_tmp: twice their number of
            // 32-byte slots; k-mers beyond the list's room are not in it (their reads are decided by kernel 3)
            const uint32_t n_list = (uint32_t)std::min<uint64_t>(n_unver, fin_anchor_ulist_cap(x->total_len));
            ktx_lg = 6;
            while ((1ull << ktx_lg) < 2ull * n_list) ktx_lg++;
            if ((e = hipMalloc(&r.d_ktx, (32ull << ktx_lg) + 32)) != hipSuccess) { (void)hipFree(d_tmp); free_replica(r); set_err(err, errlen, std::string("k-mer side table: ") + hipGetErrorString(e)); return FIN_ENODEV; }
            rc = fin_launch_build_ktx(fin_anchor_ulist(d_tmp, x->total_len), n_list, r.d_ktx, ktx_lg, nullptr);
            r.n_unverified = n_unver;
        }
        (void)hipEventRecord(t1, nullptr);
        e = hipDeviceSynchronize();
        float ms = 0; (void)hipEventElapsedTime(&ms, t0, t1); r.anchors_ms = ms;
        (void)hipEventDestroy(t0); (void)hipEventDestroy(t1);
        (void)hipFree(d_tmp);
        if (rc != 0 || e != hipSuccess) {
            free_replica(r); set_err(err, errlen, std::string("anchor table kernel: ") + (rc == (int)hipErrorOutOfMemory ? "the k-mer table filled up" : hipGetErrorString(rc ? (hipError_t)rc : e))); return FIN_ENODEV;
        }
        r.anchors_built = true;
        {   // reverse-complement pairs (for the deferred second strand): needs the prefix table of this replica
            void* d8 = nullptr;
            if (hipMalloc(&d8, 16) == hipSuccess && hipMalloc(&r.d_rcwin, fin_rcwin_bytes(x->total_len)) == hipSuccess) {
                if (fin_launch_count_rc_pairs(&d, d8, &r.n_rc_pairs, r.d_rcwin, nullptr) != 0) r.n_rc_pairs = ~0ull;   // (unknown: no deferral)
            } else r.n_rc_pairs = ~0ull;
            (void)hipFree(d8);
            if (r.n_rc_pairs == 0 || r.n_rc_pairs == ~0ull) { (void)hipFree(r.d_rcwin); r.d_rcwin = nullptr; }   // (none: the walk kernel need not look)
        }
        if (r.n_unsafe == 0) { (void)hipFree(r.d_safe); r.d_safe = nullptr; }
        if (!up_seeds) { (void)hipFree(r.d_pos); r.d_pos = nullptr; }
        d.pos = (const FinSeedEntry*)r.d_pos; d.safe = (const unsigned long long*)r.d_safe;
        d.kt3 = (const FinKt3Bucket*)r.d_kt3; d.kt3_buckets = kt3_buckets;
        d.ktx = (const FinKtxSlot*)r.d_ktx; d.ktx_log2 = ktx_lg;
    }
    d.cbf = nullptr; d.cbf_log2 = 0; d.cbf_m = 0; d.fast_path = 0; d.fbf = nullptr;
    if (d.kt3) {
        // canonical string filter (FinDevIndex::cbf): strings of m bases, 16 bits of filter per text position, a power of two of 16-byte blocks
        // (250 Mbp: 2^25 blocks, 512 MiB -- a sixteenth of the prefix table it takes the error-bridging probes from).  m = 20, or less for short
        // k: a string settles k-m+1 k-mer ends and the fast path asks three across a disagreeing base, so 3 (k-m+1) >= k must hold
        int m = (int)optv(x, O_cbf_m);
        if (m < 0) { m = (int)x->k + 1 - ((int)x->k + 2) / 3; if (m > 20) m = 20; if (m < 1) m = 1; }
        if (m > (int)x->k) m = (int)x->k;
        if (m >= 1) {
            uint32_t lg = 4;
            while ((8ull << lg) < x->total_len && lg < 31) lg++;
            if ((e = hipMalloc(&r.d_cbf, 16ull << lg)) != hipSuccess) {
                free_replica(r); set_err(err, errlen, std::string("canonical string filter: ") + hipGetErrorString(e)); return FIN_ENODEV;
            }
            if (r.lean && (e = hipMalloc(&r.d_fbf, 16ull << lg)) != hipSuccess) {
                free_replica(r); set_err(err, errlen, std::string("directional string filter: ") + hipGetErrorString(e)); return FIN_ENODEV;
            }
            const int rc = fin_launch_build_cbf(&d, r.d_cbf, r.d_fbf, lg, (uint32_t)m, nullptr);
            if (rc != 0 || (e = hipDeviceSynchronize()) != hipSuccess) {
                free_replica(r); set_err(err, errlen, std::string("canonical string filter kernel: ") + hipGetErrorString(rc ? (hipError_t)rc : e)); return FIN_ENODEV;
            }
            d.cbf = (const FinCbfBlock*)r.d_cbf; d.cbf_log2 = lg; d.cbf_m = (uint32_t)m; d.fbf = (const FinCbfBlock*)r.d_fbf;
        }
    }
    r.table_bytes = (r.d_ptab ? (sizeof(FinPrefixIval) << (2 * d.ptab_t)) : 0) + (r.d_jtab ? (sizeof(FinPrefixIval) << (2 * d.jtab_t)) : 0) +
                    (r.d_filt ? ((1ull << (2 * d.filt_f)) / 8) : 0) + (r.d_pos ? (x->n_nodes + 1) * sizeof(FinSeedEntry) : 0) +
                    (r.d_safe ? fin_anchor_safe_words(x->total_len) * 8 : 0) + (r.d_kt3 ? 32ull * d.kt3_buckets : 0) + (r.d_ktx ? (32ull << d.ktx_log2) : 0) +
                    (r.d_rcwin ? fin_rcwin_bytes(x->total_len) : 0) + (r.d_cbf ? (16ull << d.cbf_log2) : 0) + (r.d_fbf ? (16ull << d.cbf_log2) : 0) + (r.d_lcs8 ? x->lcs8.size() : 0);
    x->replicas.push_back(r);
    return FIN_OK;
}

// diagnostic (tests): {g, u} of every entry of the anchor table of the replica on `device`, 2 * n_nodes u32; FIN_EINVAL when that replica has none
int fin_index_debug_seed_table(const fin_index* x, int device, uint32_t* out, char* err, size_t errlen) {
    const fin_index::Replica* r = x ? x->replica_on(device) : nullptr;
    if (!r || !r->d_pos || !out) { set_err(err, errlen, "no seed table on that device"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipMemcpy2D(out, 8, r->d_pos, sizeof(FinSeedEntry), 8, (size_t)x->n_nodes, hipMemcpyDeviceToHost));   // {g, u} of every entry
    return FIN_OK;
}

// diagnostic (tests): a derived table of the replica on `device` as it lies in HBM -- where it is and how many bytes of its allocation are the table (the rest is padding)
static const void* debug_table_of(const fin_index* x, const fin_index::Replica& r, int what, uint64_t& bytes) {
    const FinDevIndex& d = r.dev;
    const void* p = nullptr; bytes = 0;
    switch (what) {
        case FIN_DT_PTAB: p = r.d_ptab; bytes = sizeof(FinPrefixIval) << (2 * d.ptab_t); break;
        case FIN_DT_JTAB: p = r.d_jtab; bytes = sizeof(FinPrefixIval) << (2 * d.jtab_t); break;
        case FIN_DT_FILT: p = r.d_filt; bytes = (1ull << (2 * d.filt_f)) / 8; break;
        case FIN_DT_SAFE: p = r.d_safe; bytes = (x->total_len + 63) / 64 * 8; break;
        case FIN_DT_RCWIN: p = r.d_rcwin; bytes = (x->total_len + 511) / 512; break;
        case FIN_DT_CBF: p = r.d_cbf; bytes = 16ull << d.cbf_log2; break;
        case FIN_DT_FBF: p = r.d_fbf; bytes = 16ull << d.cbf_log2; break;
        default: break;
    }
    if (!p) bytes = 0;
    return p;
}
int64_t fin_index_debug_table_bytes(const fin_index* x, int device, int what) {
    const fin_index::Replica* r = x ? x->replica_on(device) : nullptr;
    if (!r || what < FIN_DT_PTAB || what > FIN_DT_FBF) return -1;
    uint64_t bytes = 0;
    (void)debug_table_of(x, *r, what, bytes);
    return (int64_t)bytes;
}
int fin_index_debug_table(const fin_index* x, int device, int what, void* out, uint64_t out_bytes, char* err, size_t errlen) {
    if (!x || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    const fin_index::Replica* r = x->replica_on(device);
    if (!r) { set_err(err, errlen, "no replica on that device"); return FIN_EINVAL; }
    uint64_t bytes = 0;
    const void* p = debug_table_of(x, *r, what, bytes);
    if (!p) { set_err(err, errlen, "the replica on that device has no such table"); return FIN_EINVAL; }
    if (out_bytes < bytes) { set_err(err, errlen, "table buffer too small"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipMemcpy(out, p, bytes, hipMemcpyDeviceToHost));
    return FIN_OK;
}
int fin_index_string_filter_geometry(const fin_index* x, int device, uint32_t* m, uint32_t* log2_blocks) {
    const fin_index::Replica* r = x ? x->replica_on(device) : nullptr;
    if (!r) return FIN_EINVAL;
    if (m) *m = r->d_cbf ? r->dev.cbf_m : 0u;
    if (log2_blocks) *log2_blocks = r->d_cbf ? r->dev.cbf_log2 : 0u;
    return FIN_OK;
}

// diagnostic (tests): what the compact k-mer table of the replica on `device` claims about n k-mers given as their two key words (2-bit codes, first base in the low
// bits; k1 = 0 for k <= 32): out[2 i] = g, out[2 i + 1] = flags (fin_kt3_query_kernel).  FIN_EINVAL: that replica has no k-mer table
int fin_index_debug_kmer_table(const fin_index* x, int device, const uint64_t* k0, const uint64_t* k1, uint64_t n, uint32_t* out, char* err, size_t errlen) {
    const fin_index::Replica* r = x ? x->replica_on(device) : nullptr;
    if (!r || !r->d_kt3 || !k0 || !k1 || !out || n > 0x7FFFFFFFull || x->k > 64) { set_err(err, errlen, "no k-mer table on that device (or k > 64: the query takes two key words)"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(device));
    void* d0 = nullptr; void* d1 = nullptr; void* dout = nullptr;
    int rc = FIN_OK;
    if (hipMalloc(&d0, n * 8 + 8) != hipSuccess || hipMalloc(&d1, n * 8 + 8) != hipSuccess || hipMalloc(&dout, n * 8 + 8) != hipSuccess) rc = FIN_ENOMEM;
    if (rc == FIN_OK && (hipMemcpy(d0, k0, n * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d1, k1, n * 8, hipMemcpyHostToDevice) != hipSuccess)) rc = FIN_ENODEV;
    if (rc == FIN_OK && fin_launch_kt3_query(&r->dev, (const uint64_t*)d0, (const uint64_t*)d1, (uint32_t)n, dout, nullptr) != 0) rc = FIN_ENODEV;
    if (rc == FIN_OK && hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = FIN_ENODEV;
    (void)hipFree(d0); (void)hipFree(d1); (void)hipFree(dout);
    if (rc != FIN_OK) set_err(err, errlen, "k-mer table query failed");
    return rc;
}

// ---- batches --------------------------------------------------------------------------------------------------
struct fin_batch {
    const fin_index* idx = nullptr;
    FinDevIndex dev{};
    int device = -1;
    uint64_t n_reads = 0, n_kmers = 0, n_base_strands = 0, total_bases = 0;
    void* d_bases_alloc = nullptr;   // 16 guard bytes in front: the reverse strand reads 16-byte chunks ending at a read's end
    uint8_t* d_bases = nullptr; void* d_offs = nullptr; void* d_out_offs = nullptr; void* d_out = nullptr; void* d_desc = nullptr; void* d_desc2 = nullptr; void* d_packed = nullptr; void* d_pass = nullptr; void* d_seed = nullptr; size_t cap_seed = 0; uint32_t grid_blocks2 = 0, grid_blocks3 = 0, grid_blocks_probe = 0;
    uint32_t* d_work = nullptr; uint32_t grid_blocks = 0;
    void* d_text = nullptr; void* d_last_bits = nullptr; void* d_blk_sum = nullptr; void* d_blk_off = nullptr; uint64_t* d_total = nullptr;   // output text made on the device
    size_t cap_text = 0, cap_last_bits = 0, cap_blk_sum = 0, cap_blk_off = 0;
    // text modes (fin_batch_text_mode): the fast path's per-read records, and what the most recent run did with them
    void* d_frec = nullptr; void* d_seg = nullptr; size_t cap_frec = 0, cap_seg = 0;
    int text_reads_state = 0;   // since the last load: 0 not looked at, 1 every read has a k-mer, 2 one has none (fin_batch_format_text refuses)
    uint32_t n_seg = 0; bool seg_table = false;   // the text kernels' segments (fin_text.hip): a table only when a read has more than fin_text3_seg_pairs() pairs
    int text_mode = 0; bool last_frec = false, last_text_only = false, count_from_text = false;
    // records (fin_batch_records): the dense stream of the pairs of the reads the fast path did not finish
    void* d_cstream = nullptr; size_t cap_cstream = 0; uint64_t rec_stream_pairs = 0; bool rec_ready = false, rec_passthrough = false;
    // segments (fin_batch_segments): per-read counts, block sums and offsets, seg_offs[n_reads + 1] and the segments; kept and only grown
    void* d_sgm_cnt = nullptr; void* d_sgm_bsum = nullptr; void* d_sgm_boff = nullptr; void* d_sgm_offs = nullptr; void* d_sgm = nullptr;
    size_t cap_sgm_cnt = 0, cap_sgm_bsum = 0, cap_sgm_boff = 0, cap_sgm_offs = 0, cap_sgm = 0; uint64_t n_segments = 0; bool sgm_ready = false;
    // per-read summaries and the screen made from them (fin_batch_read_summaries, fin_batch_screen): kept and only grown
    void* d_rsum = nullptr; void* d_scr_bits = nullptr; void* d_scr_ids = nullptr; void* d_scr_bsum = nullptr; void* d_scr_boff = nullptr;
    size_t cap_rsum = 0, cap_scr_bits = 0, cap_scr_ids = 0, cap_scr_bsum = 0, cap_scr_boff = 0; uint64_t n_pass = 0; bool rsum_ready = false, scr_ready = false;
    // per-read classes under a labelling (fin_batch_classify): kept and only grown; cls_labels = the serial number of the labelling they were made for
    void* d_cls = nullptr; size_t cap_cls = 0; bool cls_ready = false; uint64_t cls_labels = 0;
    // per-read taxa under a taxonomy (fin_batch_taxa): kept and only grown; made for the taxonomy with serial tax_serial under these two thresholds
    void* d_tax = nullptr; size_t cap_tax = 0; bool tax_ready = false; uint64_t tax_serial = 0; uint32_t tax_min_found = 0, tax_conf = 0;
    // per-read colour rows and heads under a colour matrix (fin_batch_pseudoalign): kept and only grown; psa_words = the matrix's words per row
    void* d_psa_rows = nullptr; size_t cap_psa_rows = 0; void* d_psa_heads = nullptr; size_t cap_psa_heads = 0; bool psa_ready = false; uint32_t psa_words = 0;
    // per-fragment colour rows and heads (fin_batch_pseudoalign_paired): buffers of their own, kept and only grown; forgotten whenever the per-read rows are
    void* d_pair_rows = nullptr; size_t cap_pair_rows = 0; void* d_pair_heads = nullptr; size_t cap_pair_heads = 0; bool pair_ready = false; uint32_t pair_words = 0;
    // per-fragment geometry (fin_batch_fragments): fin_fragment[n_reads / 2], then a flag word in a 16-byte line of its own; a buffer of its own, kept and only
    // grown; forgotten wherever the read summaries are
    void* d_frag = nullptr; size_t cap_frag = 0; bool frag_ready = false;
    // the assigned rows and heads of fin_batch_assign (per read or per fragment: asg_n of them) and the bin of fin_batch_assign_bin made from them: buffers of their
    // own, kept and only grown; asg_stream = the stream the assignment was put on, which its readers follow
    void* d_asg_rows = nullptr; size_t cap_asg_rows = 0; void* d_asg_heads = nullptr; size_t cap_asg_heads = 0; bool asg_ready = false; uint32_t asg_words = 0, asg_colors = 0;
    uint64_t asg_n = 0; hipStream_t asg_stream = nullptr;
    void* d_bin_bits = nullptr; void* d_bin_ids = nullptr; void* d_bin_bsum = nullptr; void* d_bin_boff = nullptr;
    size_t cap_bin_bits = 0, cap_bin_ids = 0, cap_bin_bsum = 0, cap_bin_boff = 0; uint64_t n_bin = 0; bool bin_ready = false;
    uint64_t text_bytes = 0;
    // kernel 4: the queue counters of the most recent finished run, copied to page-locked memory behind every run: the next run launches only
    // as many stream / walk rounds as that one needed, plus one (fin_launch_search_v4's `rounds`)
    uint32_t* h_ctr = nullptr; hipEvent_t ev_ctr = nullptr; bool ctr_pending = false; uint32_t rounds_hint = 0;
    void* d_ws = nullptr; size_t cap_ws = 0; uint64_t q_slots = 0; uint32_t* d_ctr = nullptr; uint32_t grid_blocks_stream = 0, grid_blocks_walk = 0;   // kernel 4: item queues, counters
    uint32_t* d_ovf_list = nullptr; uint32_t* d_ovf_count = nullptr; uint64_t* d_ovf_scratch = nullptr;
    unsigned long long* d_count = nullptr;
    uint32_t ovf_blocks = 0;
    // HIP events of every run, recorded on the stream the step was launched on: 0 step begins (before the ingest kernel),
    // 1 reads packed + output prefilled, 2 probe pre-pass done (kernel 3), 3 search kernel done, 4 step ends (overflow redo done)
    struct RunEvents { hipEvent_t e[5]; };
    std::vector<RunEvents> runs;
    uint64_t n_chunks = 0;
    uint64_t max_read_len = 0;   // (the fused ingest takes batches of short reads only: one lane packs a read)
    bool last_fused = false;     // the most recent run's ingest was the fast pre-pass's (no pack kernel)
    int last_strands = FIN_MERGED; uint32_t last_kernel = 0, last_no_prefill = 0, last_ovf_cap = 0xFFFFFFFFu;
    int ovf_state = 0; uint32_t last_ovf = 0;   // the most recent run's overflow list: 0 not looked at yet, 1 within its capacity, 2 overran (results withheld)
    size_t cap_pass = 0, cap_bases = 0, cap_desc = 0, cap_desc2 = 0, cap_offs = 0, cap_out_offs = 0, cap_out = 0, cap_ovf_list = 0, cap_packed = 0;
    hipStream_t own_stream = nullptr;    // uploads, the pack kernel and (for the library's own pipeline) the search run here
    hipStream_t last_stream = nullptr;   // stream of the most recent fin_batch_run
    // kernel 4: the output prefill runs on a side stream beside ingest and the probe pre-pass (forked from and joined to the launch stream by events)
    hipStream_t side_stream = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool ran = false;
    std::vector<uint64_t> h_offs, h_out_offs; std::vector<FinReadDesc> h_desc, h_desc2;   // host staging of the per-read tables
};

void fin_batch_free(fin_batch* b) {
    if (!b) return;
    if (b->device >= 0) (void)hipSetDevice(b->device);
    (void)hipFree(b->d_bases_alloc); (void)hipFree(b->d_desc); (void)hipFree(b->d_desc2); (void)hipFree(b->d_packed); (void)hipFree(b->d_pass); (void)hipFree(b->d_seed); (void)hipFree(b->d_work); (void)hipFree(b->d_offs); (void)hipFree(b->d_out_offs); (void)hipFree(b->d_out);
    (void)hipFree(b->d_ws); (void)hipFree(b->d_ctr);
    if (b->h_ctr) (void)hipHostFree(b->h_ctr);
    if (b->ev_ctr) (void)hipEventDestroy(b->ev_ctr);
    (void)hipFree(b->d_cstream); (void)hipFree(b->d_frec); (void)hipFree(b->d_seg); (void)hipFree(b->d_text); (void)hipFree(b->d_last_bits); (void)hipFree(b->d_blk_sum); (void)hipFree(b->d_blk_off); (void)hipFree(b->d_total);
    (void)hipFree(b->d_sgm_cnt); (void)hipFree(b->d_sgm_bsum); (void)hipFree(b->d_sgm_boff); (void)hipFree(b->d_sgm_offs); (void)hipFree(b->d_sgm);
    (void)hipFree(b->d_rsum); (void)hipFree(b->d_scr_bits); (void)hipFree(b->d_scr_ids); (void)hipFree(b->d_scr_bsum); (void)hipFree(b->d_scr_boff); (void)hipFree(b->d_cls); (void)hipFree(b->d_tax); (void)hipFree(b->d_psa_rows); (void)hipFree(b->d_psa_heads); (void)hipFree(b->d_pair_rows); (void)hipFree(b->d_pair_heads); (void)hipFree(b->d_frag);
    (void)hipFree(b->d_asg_rows); (void)hipFree(b->d_asg_heads); (void)hipFree(b->d_bin_bits); (void)hipFree(b->d_bin_ids); (void)hipFree(b->d_bin_bsum); (void)hipFree(b->d_bin_boff);
    (void)hipFree(b->d_ovf_list); (void)hipFree(b->d_ovf_count); (void)hipFree(b->d_ovf_scratch); (void)hipFree(b->d_count);
    for (auto& r : b->runs) for (auto& e : r.e) (void)hipEventDestroy(e);
    if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
    if (b->side_stream) (void)hipStreamDestroy(b->side_stream);
    if (b->ev_fork) (void)hipEventDestroy(b->ev_fork);
    if (b->ev_join) (void)hipEventDestroy(b->ev_join);
    delete b;
}

int fin_batch_create(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, fin_batch** out,
                     char* err, size_t errlen) {
    if (!idx) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (idx->replicas.empty()) { set_err(err, errlen, "index is not resident on a device: call fin_index_to_device first (no CPU fallback)"); return FIN_ENODEV; }
    return fin_batch_create_on(idx, idx->replicas[0].device, bases, offsets, n_reads, out, err, errlen);
}

// (re)fill a batch with a read set: device buffers grow on demand and are kept, so a batch that is reloaded with read sets of
// similar size allocates once.  All copies and the pack kernel run on the batch's own stream; returns when they have finished.
// `first_base` points at base offsets[0] of the read set
static int batch_load(fin_batch* b, const char* first_base, const uint64_t* offsets, uint64_t n_reads, char* err, size_t errlen) {
    // (the kernel's work counter hands out read numbers in ranges of 64 and may overshoot by a range per wave)
    if (n_reads >= 0xFFF00000ull) { set_err(err, errlen, "more than 2^32-2^20 reads in one batch"); return FIN_ELIMIT; }
    const uint64_t base0 = offsets[0];
    const uint64_t k = b->idx->k;
    std::vector<uint64_t>& offs = b->h_offs; std::vector<uint64_t>& out_offs = b->h_out_offs;
    std::vector<FinReadDesc>& desc = b->h_desc; std::vector<FinReadDesc>& desc2 = b->h_desc2;
    offs.resize(n_reads + 1); out_offs.resize(n_reads + 1); desc.resize(n_reads + 1); desc2.resize(n_reads + 1);
    uint64_t n_chunks = 0, max_len = 0;
    out_offs[0] = 0;
    for (uint64_t r = 0; r <= n_reads; r++) offs[r] = offsets[r] - base0;
    for (uint64_t r = 0; r < n_reads; r++) {
        uint64_t len = offs[r + 1] - offs[r];
        if (len >= 0x7FFFFFFFull) { set_err(err, errlen, "read longer than 2^31-1 bases"); return FIN_ELIMIT; }
        out_offs[r + 1] = out_offs[r] + (len >= k ? len - k + 1 : 0);
        desc[r] = FinReadDesc{offs[r], (uint32_t)len, (uint32_t)out_offs[r]};
        desc2[r] = FinReadDesc{n_chunks, (uint32_t)len, (uint32_t)out_offs[r]};   // off = first packed chunk of the read
        n_chunks += 2 * ((len + 31) / 32);
        max_len = std::max<uint64_t>(max_len, len);
    }
    desc[n_reads] = FinReadDesc{offs[n_reads], 0, (uint32_t)out_offs[n_reads]};
    desc2[n_reads] = FinReadDesc{n_chunks, 0, (uint32_t)out_offs[n_reads]};
    if (out_offs[n_reads] >= 0xFFFFFFFFull) { set_err(err, errlen, "more than 2^32-1 k-mers in one batch: split the batch"); return FIN_ELIMIT; }
    if (offs[n_reads] >= 0xFFFFFFFFull) { set_err(err, errlen, "more than 2^32-1 bases in one batch: split the batch"); return FIN_ELIMIT; }
    b->n_reads = n_reads;
    b->total_bases = offs[n_reads];
    b->n_kmers = out_offs[n_reads];
    b->n_base_strands = 2 * b->total_bases;
    auto fail = [&](hipError_t e, const char* what) {
        set_err(err, errlen, std::string(what) + ": " + hipGetErrorString(e));
        b->n_reads = 0; b->n_kmers = 0; b->total_bases = 0; b->n_base_strands = 0;   // a failed load leaves an empty batch
        return FIN_ENODEV;
    };
    hipError_t e;
    if ((e = hipSetDevice(b->device)) != hipSuccess) return fail(e, "hipSetDevice");
    if (!b->own_stream && (e = hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
    hipStream_t st = b->own_stream;
    // a reload must not overtake a search that is still running on another stream
    if (b->last_stream != st && b->ran) { if ((e = hipStreamSynchronize(b->last_stream)) != hipSuccess) return fail(e, "hipStreamSynchronize"); }
    auto grow = [&](void** p, size_t& cap, size_t bytes) -> hipError_t {
        if (bytes <= cap) return hipSuccess;
        if (*p) { (void)hipStreamSynchronize(st); (void)hipFree(*p); *p = nullptr; cap = 0; }
        const size_t want = bytes + bytes / 8;   // a little head room: sub-batches of a stream of reads differ slightly in size
        hipError_t r = hipMalloc(p, want);
        if (r == hipSuccess) cap = want;
        return r;
    };
    if ((e = grow(&b->d_bases_alloc, b->cap_bases, b->total_bases + 128)) != hipSuccess) return fail(e, "hipMalloc(bases)");
    b->d_bases = (uint8_t*)b->d_bases_alloc + 64;   // guard bytes: 32-byte windows may overhang a read at either end
    if ((e = hipMemsetAsync(b->d_bases_alloc, 'N', 64, st)) != hipSuccess) return fail(e, "hipMemset(bases)");
    if ((e = hipMemsetAsync(b->d_bases + b->total_bases, 'N', 64, st)) != hipSuccess) return fail(e, "hipMemset(bases)");
    const size_t rd = (n_reads + 1);
    if ((e = grow(&b->d_desc, b->cap_desc, rd * sizeof(FinReadDesc))) != hipSuccess) return fail(e, "hipMalloc(descriptors)");
    if ((e = grow(&b->d_desc2, b->cap_desc2, rd * sizeof(FinReadDesc))) != hipSuccess) return fail(e, "hipMalloc(descriptors)");
    if ((e = grow(&b->d_offs, b->cap_offs, rd * 8)) != hipSuccess) return fail(e, "hipMalloc(offsets)");
    if ((e = grow(&b->d_out_offs, b->cap_out_offs, rd * 8)) != hipSuccess) return fail(e, "hipMalloc(out offsets)");
    if ((e = grow(&b->d_out, b->cap_out, b->n_kmers * 8 + 16)) != hipSuccess) return fail(e, "hipMalloc(output)");
    if ((e = grow((void**)&b->d_ovf_list, b->cap_ovf_list, rd * 4)) != hipSuccess) return fail(e, "hipMalloc(overflow list)");
    if ((e = grow(&b->d_packed, b->cap_packed, (n_chunks + 4) * 16)) != hipSuccess) return fail(e, "hipMalloc(packed reads)");
    if ((e = grow(&b->d_pass, b->cap_pass, (2 * rd + 4) * 4)) != hipSuccess) return fail(e, "hipMalloc(probe results)");
    if (!b->d_work && (e = hipMalloc((void**)&b->d_work, 4)) != hipSuccess) return fail(e, "hipMalloc");
    if (!b->grid_blocks2) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device) != hipSuccess || cus <= 0) cus = 256;
        b->grid_blocks2 = (uint32_t)cus * (uint32_t)fin_v2_blocks_per_cu();
        b->grid_blocks3 = (uint32_t)cus * (uint32_t)fin_v3_blocks_per_cu();
        b->grid_blocks_probe = (uint32_t)cus * (uint32_t)fin_probe_blocks_per_cu();
        b->grid_blocks_stream = (uint32_t)cus * (uint32_t)fin_stream_blocks_per_cu();
        b->grid_blocks_walk = (uint32_t)cus * (uint32_t)fin_walk_blocks_per_cu();
    }
    b->q_slots = 0;
    if (optv(b->idx, O_kernel) == 4 && n_reads < 0x0FFFFFF0ull) {   // kernel 4's item queues and its list of reads for kernel 3 (read numbers travel in 28 bits of an item's first word)
        const uint32_t maxg = std::max(std::max(b->grid_blocks_probe, b->grid_blocks_stream), b->grid_blocks_walk);
        if ((e = grow(&b->d_ws, b->cap_ws, fin_v4_workspace_bytes((uint32_t)n_reads, maxg))) != hipSuccess) return fail(e, "hipMalloc(pipeline queues)");
        if (!b->d_ctr && (e = hipMalloc((void**)&b->d_ctr, fin_v4_counter_words() * 4)) != hipSuccess) return fail(e, "hipMalloc");
        b->q_slots = fin_v4_queue_slots((uint32_t)n_reads, maxg);
        // the overflow list under kernel 4: a read can be pushed once per strand by the stream kernel (deque overflow, epoch budget) and once
        // more each time kernel 3 redoes it from its list (twice at most: either strand's walk may give the read up) -- four entries per
        // read at the very most; k > 128: the walk kernel appends to it through reserved slots, which needs kernel 3's list capacity
        const uint64_t ovf_need = std::max<uint64_t>(4 * rd + 64, fin_v4_list_slots((uint32_t)n_reads, maxg));
        if ((e = grow((void**)&b->d_ovf_list, b->cap_ovf_list, ovf_need * 4)) != hipSuccess) return fail(e, "hipMalloc(overflow list)");
        const fin_index::Replica* rp = b->idx->replica_on(b->device);
        if (rp && (rp->dev.pos || rp->lean) && (e = grow(&b->d_seed, b->cap_seed, (2 * rd + 4) * 4)) != hipSuccess) return fail(e, "hipMalloc(seed nodes)");
    }
    if (!b->d_ovf_count && (e = hipMalloc((void**)&b->d_ovf_count, 4)) != hipSuccess) return fail(e, "hipMalloc");
    if (!b->d_count && (e = hipMalloc((void**)&b->d_count, 8)) != hipSuccess) return fail(e, "hipMalloc");
    {
        uint32_t want = (uint32_t)std::min<uint64_t>(64, (n_reads + 255) / 256);
        if (want == 0) want = 1;
        if (want > b->ovf_blocks) {
            if (b->d_ovf_scratch) { (void)hipStreamSynchronize(st); (void)hipFree(b->d_ovf_scratch); b->d_ovf_scratch = nullptr; b->ovf_blocks = 0; }
            if ((e = hipMalloc((void**)&b->d_ovf_scratch, (size_t)want * 256 * fin_overflow_deque_cap() * 8)) != hipSuccess) return fail(e, "hipMalloc(overflow scratch)");
            b->ovf_blocks = want;
        }
    }
    if (b->total_bases && (e = hipMemcpyAsync(b->d_bases, first_base, b->total_bases, hipMemcpyHostToDevice, st)) != hipSuccess) return fail(e, "hipMemcpy(bases)");
    if ((e = hipMemcpyAsync(b->d_offs, offs.data(), rd * 8, hipMemcpyHostToDevice, st)) != hipSuccess) return fail(e, "hipMemcpy(offsets)");
    if ((e = hipMemcpyAsync(b->d_out_offs, out_offs.data(), rd * 8, hipMemcpyHostToDevice, st)) != hipSuccess) return fail(e, "hipMemcpy(out offsets)");
    if ((e = hipMemcpyAsync(b->d_desc, desc.data(), rd * sizeof(FinReadDesc), hipMemcpyHostToDevice, st)) != hipSuccess) return fail(e, "hipMemcpy(descriptors)");
    if ((e = hipMemcpyAsync(b->d_desc2, desc2.data(), rd * sizeof(FinReadDesc), hipMemcpyHostToDevice, st)) != hipSuccess) return fail(e, "hipMemcpy(descriptors)");
    // (the ASCII reads are what is resident: packing them to 2-bit chunks of both strands -- the reference's get_rc and base
    //  decoding, inside its timed region, search_fmin.hh:46-71 -- is the first kernel of every step, see fin_batch_run)
    b->n_chunks = n_chunks; b->max_read_len = max_len;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(e, "upload");
    b->ran = false; b->last_stream = nullptr; b->sgm_ready = false; b->rsum_ready = false; b->scr_ready = false; b->frag_ready = false; b->cls_ready = false; b->tax_ready = false; b->psa_ready = false; b->pair_ready = false; b->asg_ready = false; b->bin_ready = false;
    b->rounds_hint = 0; b->ctr_pending = false;   // (new reads: nothing is known about the rounds they need)
    b->text_reads_state = 0;
    return FIN_OK;
}

int fin_batch_create_on(const fin_index* idx, int device, const char* bases, const uint64_t* offsets, uint64_t n_reads, fin_batch** out,
                        char* err, size_t errlen) {
    if (!idx || !offsets || !out || (n_reads && !bases)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    const fin_index::Replica* rep = idx->replica_on(device);
    if (!rep) { set_err(err, errlen, "index is not resident on that device: call fin_index_to_device first (no CPU fallback)"); return FIN_ENODEV; }
    fin_batch* b = new (std::nothrow) fin_batch();
    if (!b) { set_err(err, errlen, "out of memory"); return FIN_ENOMEM; }
    b->idx = idx; b->dev = rep->dev; b->device = device;
    const int rc = batch_load(b, bases ? bases + offsets[0] : nullptr, offsets, n_reads, err, errlen);
    if (rc != FIN_OK) { fin_batch_free(b); return rc; }
    *out = b;
    return FIN_OK;
}

int fin_batch_reload(fin_batch* b, const char* bases, const uint64_t* offsets, uint64_t n_reads, char* err, size_t errlen) {
    if (!b || !offsets || (n_reads && !bases)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    return batch_load(b, bases ? bases + offsets[0] : nullptr, offsets, n_reads, err, errlen);
}

int fin_batch_run(fin_batch* b, int strands, void* hip_stream, char* err, size_t errlen) {
    if (!b || (strands != FIN_FWD && strands != FIN_MERGED)) { set_err(err, errlen, "bad argument"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (b->runs.size() >= 1024) {   // a long-lived batch keeps the most recent launches only
        for (auto& e : b->runs.front().e) (void)hipEventDestroy(e);
        b->runs.erase(b->runs.begin());
    }
    fin_batch::RunEvents ev;
    for (auto& e : ev.e) HIPCHK(hipEventCreate(&e));
    b->runs.push_back(ev);
    b->last_strands = strands;
    b->last_stream = st; b->ran = true;
    // ---- one step of the hot path, everything on `st`: ingest (ASCII -> 2-bit chunks of both strands), output prefill, probe
    //      pre-pass, search kernel, overflow redo ----
    HIPCHK(hipEventRecord(ev.e[0], st));
    b->dev.budget_mult = (uint32_t)optv(b->idx, O_epoch_budget_mult); b->dev.budget_add = (uint32_t)optv(b->idx, O_epoch_budget_add);
    b->dev.ovf_cap = (uint32_t)std::min<uint64_t>(b->cap_ovf_list / 4, 0xFFFFFFFFull);
    if (const int64_t forced = optv(b->idx, O_debug_ovf_cap)) b->dev.ovf_cap = (uint32_t)std::min<int64_t>(forced, (int64_t)b->dev.ovf_cap);   // (tests: a tiny list)
    b->last_ovf_cap = b->dev.ovf_cap; b->ovf_state = 0; b->rec_ready = false; b->sgm_ready = false; b->rsum_ready = false; b->scr_ready = false; b->frag_ready = false; b->cls_ready = false; b->tax_ready = false; b->psa_ready = false; b->pair_ready = false; b->asg_ready = false; b->bin_ready = false;
    b->dev.pp_seg = (uint32_t)optv(b->idx, O_debug_pp_seg);
    b->dev.pp_max_len = (uint32_t)std::min<uint64_t>(b->max_read_len, 0xFFFFFFFFull);
    b->dev.pp_park = (uint32_t)optv(b->idx, O_pp_park);
    b->dev.pp_wide_out = (uint32_t)optv(b->idx, O_pp_wide_out);
    b->dev.pp_park_cap = (uint32_t)(int32_t)optv(b->idx, O_debug_pp_park_cap);
    b->dev.lean_walk = (uint32_t)optv(b->idx, O_lean_walk);
    {   // text re-anchoring needs the upload's verdict on every text place (the bitmap, or the knowledge that all are safe); the anchor table
        // is used when it exists, text re-anchoring is on (seeds are verified by its comparison) and the batch has room for seed nodes
        const fin_index::Replica* rep = b->idx->replica_on(b->device);
        b->dev.text_anchors = (optv(b->idx, O_text_anchors) && rep && rep->anchors_built) ? 1u : 0u;
        b->dev.safe = rep ? rep->dev.safe : nullptr;
        b->dev.pos = (optv(b->idx, O_seed_anchors) && b->dev.text_anchors && b->d_seed && rep) ? rep->dev.pos : nullptr;
        b->dev.filt = (optv(b->idx, O_filt_f) != 0 && rep) ? rep->dev.filt : nullptr;
        const bool lean = rep && rep->lean && optv(b->idx, O_seed_anchors) && b->dev.text_anchors && b->d_seed && optv(b->idx, O_kmer_table) && rep->dev.fbf;
        b->dev.fbf = lean ? rep->dev.fbf : nullptr;
        b->dev.kt3 = (optv(b->idx, O_kmer_table) && rep && (b->dev.pos || lean)) ? rep->dev.kt3 : nullptr;
        b->dev.ktx = (b->dev.kt3 && rep) ? rep->dev.ktx : nullptr; b->dev.ktx_log2 = rep ? rep->dev.ktx_log2 : 0;
        b->dev.cbf = (rep && b->dev.kt3) ? rep->dev.cbf : nullptr;
        b->dev.fast_path = (optv(b->idx, O_fast_path) && b->dev.cbf) ? 1u : 0u;
    }
    int rc = 0;
    hipEvent_t out_ready = nullptr;
    // k > 128: kernels 2 and 3 (and kernel 4's stream kernel) read 7-bit LCS values and cannot run; kernel 4 can when the index has a seed
    // table (its walk kernel needs no LCS, what it cannot finish goes to the plain kernel), else the plain kernel does everything
    const int opt_kernel = (int)optv(b->idx, O_kernel);
    const uint32_t lds_limit = (uint32_t)optv(b->idx, O_lds_deque_limit);
    int kern = opt_kernel;
    if (b->dev.k > FIN_FAST_K)
        kern = (opt_kernel == 4 && b->q_slots && fin_v4_writes_gaps(&b->dev, (const uint32_t*)b->d_seed)) ? 4 : 0;
    // kernel 4 on an index with a seed table: no prefill at all, the pipeline writes every slot once (option "write_gaps")
    const int no_prefill = (kern == 4 && b->q_slots && optv(b->idx, O_write_gaps) && fin_v4_writes_gaps(&b->dev, (const uint32_t*)b->d_seed)) ? 1 : 0;
    {   // the second strand of a read only where the first left slots open: kernel 4 writing every slot itself, both strands asked for, and an
        // the second strand of a read only where the first left slots open (CHANGELOG.md 4.14): exact on any index -- a first strand that reports
        // through the streaming search or a whole-k-mer look-up (a place that may not spell the k-mer: duplicated k-mers), or from a text
        // window with a k-mer whose reverse complement is in the index too (rcwin), has its sister searched in full ("tainted")
        const fin_index::Replica* rep = b->idx->replica_on(b->device);
        b->dev.defer_ok = (kern == 4 && no_prefill && strands == FIN_MERGED && optv(b->idx, O_defer_strand) && rep && rep->anchors_built &&
                           rep->n_rc_pairs != ~0ull && (b->dev.pos || b->dev.fbf)) ? 1u : 0u;
        b->dev.rcwin = (b->dev.defer_ok && rep->d_rcwin) ? (const uint8_t*)rep->d_rcwin : nullptr;
    }
    b->last_kernel = (uint32_t)((kern == 4 && !b->q_slots) ? 3 : kern); b->last_no_prefill = (uint32_t)no_prefill;
    if (!(b->dev.defer_ok && b->dev.kt3 && (b->dev.k <= 63 || optv(b->idx, O_fast_path) >= 2))) b->dev.fast_path = 0u;   // (the fast path rides on the pair pre-pass's k-mer-table looks)
    b->dev.frec = nullptr; b->dev.text_only = 0u; b->last_frec = false; b->last_text_only = false; b->count_from_text = false;
    if (b->text_mode && kern == 4 && b->q_slots && b->dev.fast_path && no_prefill && strands == FIN_MERGED && b->n_reads) {
        // text modes: a zeroed record per read, filled by the fast path for the reads it finishes (a record that stays zero: the read's pairs are in d_out)
        if (b->cap_frec < b->n_reads * sizeof(FinFastRec)) {
            if (b->d_frec) { HIPCHK(hipStreamSynchronize(st)); (void)hipFree(b->d_frec); b->d_frec = nullptr; b->cap_frec = 0; }
            const size_t want = (b->n_reads + b->n_reads / 8 + 16) * sizeof(FinFastRec);
            if (hipMalloc(&b->d_frec, want) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "out of device memory (fast-path records)"); return FIN_ENOMEM; }
            b->cap_frec = want;
        }
        HIPCHK(hipMemsetAsync(b->d_frec, 0, b->n_reads * sizeof(FinFastRec), st));
        b->dev.frec = (FinFastRec*)b->d_frec; b->dev.text_only = b->text_mode == 2 ? 1u : 0u;
        b->last_frec = true; b->last_text_only = b->text_mode == 2;
    }
    if (kern == 4 && b->q_slots && optv(b->idx, O_overlap_prefill) && !no_prefill) {
        // fork: (-1,-1) into every output slot on the side stream, beside the pack kernel and the pre-pass (which do not touch the output);
        // the pipeline's first writer waits for ev_join.  Everything stays inside the step's bracket e[0] .. e[4] on the launch stream.
        if (!b->side_stream) {
            HIPCHK(hipStreamCreateWithFlags(&b->side_stream, hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&b->ev_join, hipEventDisableTiming));
        }
        HIPCHK(hipEventRecord(b->ev_fork, st));
        HIPCHK(hipStreamWaitEvent(b->side_stream, b->ev_fork, 0));
        HIPCHK(hipMemsetAsync(b->d_out, 0xFF, b->n_kmers * 8, b->side_stream));
        HIPCHK(hipEventRecord(b->ev_join, b->side_stream));
        out_ready = b->ev_join;
    }
    // the fused ingest: kernel 4's pair pre-pass runs a fast kernel (merged strands, deferral, its fast path writing the pairs) and every read is
    // short enough for one lane to pack it -- then that kernel reads the ASCII itself and writes the chunks of the reads it does not finish, the
    // only ones any later kernel reads (the chunks of a FIN_PASS_DONE read are undefined; every run ingests its reads again)
    const bool fused = kern == 4 && b->q_slots && optv(b->idx, O_fused_ingest) && strands == FIN_MERGED && b->dev.defer_ok && no_prefill && b->dev.fast_path &&
                       fin_pair_prepass_fuses(&b->dev) && b->max_read_len <= 32u * FIN_FAST_CHUNKS;
    b->last_fused = fused;
    if (kern != 0 && !fused)
        rc = fin_launch_pack_reads(b->d_bases, (const uint64_t*)b->d_offs, (const FinReadDesc*)b->d_desc2, b->d_packed, (uint32_t)b->n_reads, b->n_chunks, st);
    if (rc != 0) { set_err(err, errlen, std::string("pack kernel launch failed: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    if (kern == 0)
        rc = fin_launch_search_v0(&b->dev, (const uint8_t*)b->d_bases, (const uint64_t*)b->d_offs, (const uint64_t*)b->d_out_offs,
                                  b->d_out, (uint32_t)b->n_reads, strands, lds_limit, b->d_ovf_list, b->d_ovf_count, b->d_ovf_scratch,
                                  b->ovf_blocks, st, ev.e[1], ev.e[3]);
    else if (kern == 4 && b->q_slots) {
        if (b->ctr_pending && b->ev_ctr && hipEventQuery(b->ev_ctr) == hipSuccess) {   // the counters of an earlier run of these reads have arrived
            uint32_t last = 0;
            for (uint32_t r = 0; r < fin_v4_max_rounds(); r++) if (b->h_ctr[6 + 4 * r] || b->h_ctr[7 + 4 * r]) last = r;
            b->rounds_hint = std::min<uint32_t>(fin_v4_max_rounds(), std::max<uint32_t>(2u, last + 2u));
            b->ctr_pending = false;
        } else (void)hipGetLastError();
        rc = fin_launch_search_v4(&b->dev, (const uint8_t*)b->d_bases, b->d_packed, (const FinReadDesc*)b->d_desc2, (const uint64_t*)b->d_offs,
                                  (const uint64_t*)b->d_out_offs, b->d_out, b->n_kmers, (uint32_t)b->n_reads, strands, lds_limit,
                                  b->d_ovf_list, b->d_ovf_count, b->d_ovf_scratch, b->ovf_blocks, (uint32_t*)b->d_pass, (uint32_t*)b->d_seed, b->d_ws, b->q_slots, b->d_ctr,
                                  b->grid_blocks_probe, b->grid_blocks_stream, b->grid_blocks_walk, b->grid_blocks3, st, ev.e[1], ev.e[3], ev.e[2], out_ready, no_prefill,
                                  b->rounds_hint ? b->rounds_hint : fin_v4_max_rounds(), fused ? 1 : 0);
    } else if (kern == 3 || kern == 4)   // (4 without queues: selected after this batch was loaded, or too many reads for the 29 bits a read number has in an item)
        rc = fin_launch_search_v3(&b->dev, (const uint8_t*)b->d_bases, b->d_packed, (const FinReadDesc*)b->d_desc2, (const uint64_t*)b->d_offs,
                                  (const uint64_t*)b->d_out_offs, b->d_out, b->n_kmers, (uint32_t)b->n_reads, strands,
                                  lds_limit, b->d_ovf_list, b->d_ovf_count, b->d_work, b->d_ovf_scratch, b->ovf_blocks,
                                  b->grid_blocks3, optv(b->idx, O_probe_prepass) ? (uint32_t*)b->d_pass : nullptr, b->grid_blocks_probe, st, ev.e[1], ev.e[3], ev.e[2]);
    else
        rc = fin_launch_search_v2(&b->dev, (const uint8_t*)b->d_bases, b->d_packed, (const FinReadDesc*)b->d_desc2, (const uint64_t*)b->d_offs,
                                  (const uint64_t*)b->d_out_offs, b->d_out, b->n_kmers, (uint32_t)b->n_reads, strands,
                                  lds_limit, b->d_ovf_list, b->d_ovf_count, b->d_work, b->d_ovf_scratch, b->ovf_blocks,
                                  b->grid_blocks2, st, ev.e[1], ev.e[3]);
    if (rc != 0) { set_err(err, errlen, std::string("kernel launch failed: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    HIPCHK(hipEventRecord(ev.e[4], st));
    if (kern == 4 && b->q_slots && b->d_ctr && !b->ctr_pending) {   // behind the step: this run's queue counters for the next run's round count
        if (!b->h_ctr) { HIPCHK(hipHostMalloc((void**)&b->h_ctr, fin_v4_counter_words() * 4, hipHostMallocDefault)); HIPCHK(hipEventCreateWithFlags(&b->ev_ctr, hipEventDisableTiming)); }
        HIPCHK(hipMemcpyAsync(b->h_ctr, b->d_ctr, fin_v4_counter_words() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(b->ev_ctr, st));
        b->ctr_pending = true;
    }
    return FIN_OK;
}

// diagnostic (tests of the stream contract): the side stream of option "overlap_prefill", made here if no run has made it yet
void* fin_batch_debug_side_stream(fin_batch* b) {
    if (!b || hipSetDevice(b->device) != hipSuccess) return nullptr;
    if (!b->side_stream) {
        if (hipStreamCreateWithFlags(&b->side_stream, hipStreamNonBlocking) != hipSuccess) { b->side_stream = nullptr; return nullptr; }
        if (hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&b->ev_join, hipEventDisableTiming) != hipSuccess) return nullptr;
    }
    return (void*)b->side_stream;
}

uint64_t fin_batch_n_kmers(const fin_batch* b) { return b ? b->n_kmers : 0; }
uint64_t fin_batch_n_base_strands(const fin_batch* b) { return b ? (b->last_strands == FIN_MERGED ? b->n_base_strands : b->total_bases) : 0; }
void* fin_batch_device_pairs(const fin_batch* b) { return b ? b->d_out : nullptr; }

// diagnostic (tests of the text formatter): overwrite the batch's device pairs with n_kmers pairs from the host
int fin_batch_set_pairs(fin_batch* b, const int32_t* pairs, char* err, size_t errlen) {
    if (!b || !pairs) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    if (b->last_stream) HIPCHK(hipStreamSynchronize(b->last_stream));
    HIPCHK(hipMemcpy(b->d_out, pairs, (size_t)b->n_kmers * 8, hipMemcpyHostToDevice));
    b->last_frec = false; b->last_text_only = false; b->count_from_text = false; b->sgm_ready = false; b->rsum_ready = false; b->scr_ready = false; b->frag_ready = false; b->cls_ready = false; b->tax_ready = false; b->psa_ready = false; b->pair_ready = false; b->asg_ready = false; b->bin_ready = false;   // (the records of the last run say nothing about these pairs)
    return FIN_OK;
}

// diagnostic (tests of the record consumers): overwrite the records of the most recent run -- and, optionally, its pairs -- with hand-made ones.  Everything a
// kernel trusts is checked here, on the host, before a byte is copied (include/finito_amd.h); no kernel is launched
int fin_batch_set_records(fin_batch* b, const fin_read_record* recs, const int32_t* pairs, char* err, size_t errlen) {
    if (!b || !recs) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (!b->ran || !b->last_frec || !b->d_frec) {
        set_err(err, errlen, "the most recent run left no records (kernel 4, merged strands, fast path on, text mode 1 or 2): there is nothing to overwrite");
        return FIN_EINVAL;
    }
    const uint32_t k = b->dev.k;
    for (uint64_t r = 0; r < b->n_reads; r++) {
        const fin_read_record& R = recs[r];
        const uint64_t nk = b->h_out_offs[r + 1] - b->h_out_offs[r];
        const uint32_t kind = R.meta >> 16;
        const char* what = nullptr;
        if (kind > 2u) what = "a kind that is not 0, 1 or 2";
        else if (kind == 0u) {
            if (R.u || R.off0 || R.meta || R.nk || R.Es || R.Es2) what = "a kind-0 record that is not all zero (the device tells a finished read by meta >> 16 != 0)";
        } else if (R.nk != nk || nk == 0) what = "nk is not the read's number of k-mers, or the read has none";
        else if (kind == 1u) {
            const uint32_t nE = R.meta & 0xFFu;
            if (nE > 8u) what = "more than eight positions";
            uint32_t prev = 0;
            for (uint32_t e = 0; e < 8u && !what; e++) {
                const uint32_t E = (uint32_t)((e < 4u ? R.Es : R.Es2) >> (16u * (e & 3u))) & 0xFFFFu;
                if (e >= nE) { if (E) what = "an unused position field that is not zero"; continue; }
                if (E < prev) what = "positions that do not ascend";
                else if ((uint64_t)E >= nk + k - 1u) what = "a position at or beyond nk + k - 1";
                prev = E;
            }
        }
        if (what) { set_err(err, errlen, "record " + std::to_string(r) + ": " + what); return FIN_EINVAL; }
    }
    HIPCHK(hipSetDevice(b->device));
    if (b->last_stream) HIPCHK(hipStreamSynchronize(b->last_stream));
    if (b->n_reads) HIPCHK(hipMemcpy(b->d_frec, recs, (size_t)b->n_reads * sizeof(FinFastRec), hipMemcpyHostToDevice));
    if (pairs && b->n_kmers) HIPCHK(hipMemcpy(b->d_out, pairs, (size_t)b->n_kmers * 8, hipMemcpyHostToDevice));
    // last_frec / last_text_only stay as the run left them (a text-only batch still refuses its pairs); whatever was made from the old records goes
    b->count_from_text = false; b->text_bytes = 0; b->sgm_ready = false; b->n_segments = 0; b->rsum_ready = false; b->scr_ready = false; b->frag_ready = false; b->cls_ready = false; b->tax_ready = false; b->psa_ready = false; b->pair_ready = false; b->asg_ready = false; b->bin_ready = false;
    b->rec_ready = false; b->rec_passthrough = false; b->rec_stream_pairs = 0;
    return FIN_OK;
}

// (a push beyond the overflow list's capacity is dropped on the device -- fin_ovf_push -- and that read would keep a partial
//  result: the list is sized so that this cannot happen, and if it ever does NO entry point delivers results of that run -- pairs, ranges or text)
static int batch_overrun_check(fin_batch* b, hipStream_t st, char* err, size_t errlen) {
    if (!b->ran || !b->d_ovf_count) return FIN_OK;
    if (b->ovf_state == 0) {
        uint32_t ovf = 0;
        HIPCHK(hipMemcpyAsync(&ovf, b->d_ovf_count, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        b->last_ovf = ovf; b->ovf_state = ovf > b->last_ovf_cap ? 2 : 1;
    }
    if (b->ovf_state == 2) { set_err(err, errlen, "the overflow list of this batch overran (" + std::to_string(b->last_ovf) + " entries, room for " + std::to_string(b->last_ovf_cap) + "): results withheld"); return FIN_ELIMIT; }
    return FIN_OK;
}

int fin_batch_download(fin_batch* b, int32_t* pairs_out, uint64_t* n_positive, char* err, size_t errlen) {
    if (!b) { set_err(err, errlen, "null batch"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    // everything below is ordered behind the most recent search by running on its stream
    hipStream_t st = b->ran ? b->last_stream : b->own_stream;
    if (b->ran && b->last_text_only && (pairs_out || (n_positive && !b->count_from_text))) {
        set_err(err, errlen, "this batch ran in text-only mode (fin_batch_text_mode 2): the pairs of the reads its fast path finished were never written; "
                             "the number of found pairs is known once fin_batch_format_text has run");
        return FIN_EINVAL;
    }
    if (n_positive && b->n_kmers && !b->count_from_text) {
        int rc = fin_launch_count_positive(b->d_out, b->n_kmers, b->d_count, st);
        if (rc != 0) { set_err(err, errlen, std::string("count kernel: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    }
    if (const int orc = batch_overrun_check(b, st, err, errlen)) return orc;
    if (pairs_out && b->n_kmers) HIPCHK(hipMemcpyAsync(pairs_out, b->d_out, b->n_kmers * 8, hipMemcpyDeviceToHost, st));
    unsigned long long c = 0;
    if (n_positive && b->n_kmers) HIPCHK(hipMemcpyAsync(&c, b->d_count, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_positive) *n_positive = c;
    return FIN_OK;
}

int fin_batch_download_range(fin_batch* b, uint64_t first_pair, uint64_t n_pairs, int32_t* pairs_out, char* err, size_t errlen) {
    if (!b || (n_pairs && !pairs_out)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (first_pair > b->n_kmers || n_pairs > b->n_kmers - first_pair) { set_err(err, errlen, "pair range outside the batch"); return FIN_EINVAL; }
    if (b->ran && b->last_text_only) { set_err(err, errlen, "this batch ran in text-only mode (fin_batch_text_mode 2): its pairs are not materialised"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->ran ? b->last_stream : b->own_stream;
    if (const int orc = batch_overrun_check(b, st, err, errlen)) return orc;
    if (n_pairs) HIPCHK(hipMemcpyAsync(pairs_out, (const char*)b->d_out + first_pair * 8, n_pairs * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FIN_OK;
}

// ---- the output text, made on the device --------------------------------------------------------------------------------------
static int batch_grow(fin_batch* b, void** p, size_t& cap, size_t bytes, hipStream_t st) {
    if (bytes <= cap) return FIN_OK;
    if (*p) { (void)hipStreamSynchronize(st); (void)hipFree(*p); *p = nullptr; cap = 0; }
    const size_t want = bytes + bytes / 8 + 256;
    if (hipMalloc(p, want) != hipSuccess) return FIN_ENOMEM;
    cap = want;
    return FIN_OK;
}

int fin_batch_format_text(fin_batch* b, uint64_t* text_bytes, char* err, size_t errlen) {
    if (!b) { set_err(err, errlen, "null batch"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->ran ? b->last_stream : b->own_stream;
    if (const int orc = batch_overrun_check(b, st, err, errlen)) return orc;
    if (b->text_reads_state == 0) {   // once per load: every read needs a pair to hang its line on; the segments of the record path
        b->text_reads_state = 1;
        const uint64_t SEG = fin_text3_seg_pairs();
        uint64_t n_seg = 0; bool longer = false;
        for (uint64_t r = 0; r < b->n_reads; r++) {
            const uint64_t nk = b->h_out_offs[r + 1] - b->h_out_offs[r];
            if (nk == 0) { b->text_reads_state = 2; break; }
            n_seg += (nk + SEG - 1) / SEG; longer = longer || nk > SEG;
        }
        b->seg_table = false; b->n_seg = (uint32_t)b->n_reads;
        if (b->text_reads_state == 1 && longer) {
            std::vector<uint32_t> seg; seg.reserve(2 * n_seg);
            for (uint64_t r = 0; r < b->n_reads; r++) {
                const uint64_t nk = b->h_out_offs[r + 1] - b->h_out_offs[r];
                for (uint64_t f = 0; f < nk; f += SEG) { seg.push_back((uint32_t)r); seg.push_back((uint32_t)f); }
            }
            if (batch_grow(b, &b->d_seg, b->cap_seg, seg.size() * 4, st)) { b->text_reads_state = 0; set_err(err, errlen, "out of device memory (text segments)"); return FIN_ENOMEM; }
            HIPCHK(hipMemcpyAsync(b->d_seg, seg.data(), seg.size() * 4, hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));
            b->seg_table = true; b->n_seg = (uint32_t)n_seg;
        }
    }
    if (b->text_reads_state == 2) { set_err(err, errlen, "a read without k-mers: its empty line belongs to no pair (format such batches on the host)"); return FIN_EINVAL; }
    const uint32_t nb = fin_text_blocks(b->n_kmers);
    if (b->ran && b->last_frec) {
        // the run left fast-path records: the finished reads' pairs are made from them again (in text-only mode they exist nowhere else), the
        // length pass counts the found pairs on its way
        if (batch_grow(b, &b->d_blk_sum, b->cap_blk_sum, (size_t)b->n_seg * 4 + 4, st) ||
            batch_grow(b, &b->d_blk_off, b->cap_blk_off, (size_t)fin_text3_off_words(b->n_seg) * 8 + 8, st)) { set_err(err, errlen, "out of device memory (text tables)"); return FIN_ENOMEM; }
        if (!b->d_total) HIPCHK(hipMalloc((void**)&b->d_total, 8));
        HIPCHK(hipMemsetAsync(b->d_count, 0, 8, st));
        const void* seg = b->seg_table ? b->d_seg : nullptr;
        int rc = fin_launch_text3_lengths(b->d_out, (const uint64_t*)b->d_out_offs, b->d_frec, seg, b->n_seg, b->dev.k, (uint32_t*)b->d_blk_sum, (uint64_t*)b->d_blk_off, b->d_total, b->d_count, st);
        if (rc != 0) { set_err(err, errlen, std::string("text kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
        uint64_t total = 0;
        HIPCHK(hipMemcpyAsync(&total, b->d_total, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (batch_grow(b, &b->d_text, b->cap_text, (size_t)total + 16, st)) { set_err(err, errlen, "out of device memory (text)"); return FIN_ENOMEM; }
        rc = fin_launch_text3_write(b->d_out, (const uint64_t*)b->d_out_offs, b->d_frec, seg, b->n_seg, b->dev.k, (const uint64_t*)b->d_blk_off, (char*)b->d_text, st);
        if (rc != 0) { set_err(err, errlen, std::string("text kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
        b->count_from_text = true;
        b->text_bytes = total;
        if (text_bytes) *text_bytes = total;
        return FIN_OK;
    }
    if (batch_grow(b, &b->d_last_bits, b->cap_last_bits, ((b->n_kmers + 31) / 32 + 1) * 4, st) || batch_grow(b, &b->d_blk_sum, b->cap_blk_sum, (size_t)nb * 4 + 4, st) ||
        batch_grow(b, &b->d_blk_off, b->cap_blk_off, (size_t)fin_text_off_words(b->n_kmers) * 8 + 8, st)) { set_err(err, errlen, "out of device memory (text tables)"); return FIN_ENOMEM; }
    if (!b->d_total) HIPCHK(hipMalloc((void**)&b->d_total, 8));
    int rc = fin_launch_text_lengths(b->d_out, b->n_kmers, (const uint64_t*)b->d_out_offs, (uint32_t)b->n_reads, (uint32_t*)b->d_last_bits, (uint32_t*)b->d_blk_sum,
                                     (uint64_t*)b->d_blk_off, b->d_total, st);
    if (rc != 0) { set_err(err, errlen, std::string("text kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, b->d_total, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (batch_grow(b, &b->d_text, b->cap_text, (size_t)total + 16, st)) { set_err(err, errlen, "out of device memory (text)"); return FIN_ENOMEM; }
    rc = fin_launch_text_write(b->d_out, b->n_kmers, (const uint64_t*)b->d_blk_off, (const uint32_t*)b->d_last_bits, (char*)b->d_text, st);
    if (rc != 0) { set_err(err, errlen, std::string("text kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    b->text_bytes = total;
    if (text_bytes) *text_bytes = total;
    return FIN_OK;
}

int fin_batch_text_mode(fin_batch* b, int mode) {
    if (!b || mode < 0 || mode > 2) return FIN_EINVAL;
    b->text_mode = mode;
    return FIN_OK;
}

int fin_batch_download_text(fin_batch* b, char* text_out, char* err, size_t errlen) {
    if (!b || (b->text_bytes && !text_out)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->ran ? b->last_stream : b->own_stream;
    if (const int orc = batch_overrun_check(b, st, err, errlen)) return orc;
    if (b->text_bytes) HIPCHK(hipMemcpyAsync(text_out, b->d_text, b->text_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FIN_OK;
}

// ---- results as records (fin_records.hip) --------------------------------------------------------------------------------------
int fin_batch_records(fin_batch* b, uint64_t* n_stream_pairs, char* err, size_t errlen) {
    if (!b || !b->ran) { set_err(err, errlen, "no run to take records from"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    if (const int orc = batch_overrun_check(b, st, err, errlen)) return orc;
    if (!b->last_frec) {
        // the run left no fast-path records (forward-only search, fast path off or not applicable, text mode 0): every read's pairs are in the batch's
        // output as they stand -- that IS the stream, and every record says "nk pairs follow"
        b->rec_passthrough = true; b->rec_stream_pairs = b->n_kmers; b->rec_ready = true;
        if (n_stream_pairs) *n_stream_pairs = b->n_kmers;
        return FIN_OK;
    }
    const uint32_t nb = fin_rec_blocks((uint32_t)b->n_reads);
    if (batch_grow(b, &b->d_blk_sum, b->cap_blk_sum, (size_t)nb * 4 + 4, st) || batch_grow(b, &b->d_blk_off, b->cap_blk_off, (size_t)nb * 8 + 8, st)) { set_err(err, errlen, "out of device memory (record tables)"); return FIN_ENOMEM; }
    if (!b->d_total) HIPCHK(hipMalloc((void**)&b->d_total, 8));
    int rc = fin_launch_rec_count(b->d_frec, (const uint64_t*)b->d_out_offs, (uint32_t)b->n_reads, (uint32_t*)b->d_blk_sum, (uint64_t*)b->d_blk_off, b->d_total, st);
    if (rc != 0) { set_err(err, errlen, std::string("record kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, b->d_total, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (batch_grow(b, &b->d_cstream, b->cap_cstream, (size_t)total * 8 + 16, st)) { set_err(err, errlen, "out of device memory (pair stream)"); return FIN_ENOMEM; }
    rc = fin_launch_rec_compact(b->d_frec, (const uint64_t*)b->d_out_offs, b->d_out, (uint32_t)b->n_reads, (const uint64_t*)b->d_blk_off, b->d_cstream, st);
    if (rc != 0) { set_err(err, errlen, std::string("record kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    b->rec_passthrough = false; b->rec_stream_pairs = total; b->rec_ready = true;
    if (n_stream_pairs) *n_stream_pairs = total;
    return FIN_OK;
}

int fin_batch_download_records(fin_batch* b, fin_read_record* recs_out, int32_t* stream_pairs_out, char* err, size_t errlen) {
    if (!b || !b->rec_ready || (b->n_reads && !recs_out) || (b->rec_stream_pairs && !stream_pairs_out)) { set_err(err, errlen, "fin_batch_records first; null buffer"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    if (b->rec_passthrough) {
        if (b->n_kmers) HIPCHK(hipMemcpyAsync(stream_pairs_out, b->d_out, b->n_kmers * 8, hipMemcpyDeviceToHost, st));
        for (uint64_t r = 0; r < b->n_reads; r++) recs_out[r] = fin_read_record{0u, 0u, 0u, (uint32_t)(b->h_out_offs[r + 1] - b->h_out_offs[r]), 0ull, 0ull};
    } else {
        static_assert(sizeof(fin_read_record) == sizeof(FinFastRec), "the public record is the device's");
        if (b->n_reads) HIPCHK(hipMemcpyAsync(recs_out, b->d_frec, b->n_reads * sizeof(FinFastRec), hipMemcpyDeviceToHost, st));
        if (b->rec_stream_pairs) HIPCHK(hipMemcpyAsync(stream_pairs_out, b->d_cstream, b->rec_stream_pairs * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return FIN_OK;
}

// ---- results as segments (fin_segments.hip) ---------------------------------------------------------------------------------------
static_assert(sizeof(fin_segment) == 16, "a segment is 16 bytes");

int fin_batch_segments(fin_batch* b, uint64_t* n_segments, char* err, size_t errlen) {
    if (!b) { set_err(err, errlen, "null batch"); return FIN_EINVAL; }
    if (!b->ran) { set_err(err, errlen, "this batch has not run: there is nothing to make segments of (fin_batch_run first)"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    b->sgm_ready = false;
    if (b->n_kmers == 0) {   // no read has a k-mer (the step searched nothing: there is no overflow list to look at): every read owns no segment
        if (batch_grow(b, &b->d_sgm_offs, b->cap_sgm_offs, (size_t)b->n_reads * 8 + 8, st)) { set_err(err, errlen, "out of device memory (segment tables)"); return FIN_ENOMEM; }
        HIPCHK(hipMemsetAsync(b->d_sgm_offs, 0, (size_t)b->n_reads * 8 + 8, st));
        HIPCHK(hipStreamSynchronize(st));
        b->n_segments = 0; b->sgm_ready = true;
        if (n_segments) *n_segments = 0;
        return FIN_OK;
    }
    if (const int orc = batch_overrun_check(b, st, err, errlen)) return orc;   // a run without results: nothing is written
    const uint32_t nr = (uint32_t)b->n_reads, nb = fin_sgm_blocks(nr);
    if (batch_grow(b, &b->d_sgm_offs, b->cap_sgm_offs, (size_t)nr * 8 + 8, st) || batch_grow(b, &b->d_sgm_cnt, b->cap_sgm_cnt, (size_t)nr * 4 + 4, st) ||
        batch_grow(b, &b->d_sgm_bsum, b->cap_sgm_bsum, (size_t)nb * 4 + 4, st) || batch_grow(b, &b->d_sgm_boff, b->cap_sgm_boff, (size_t)nb * 8 + 8, st)) {
        set_err(err, errlen, "out of device memory (segment tables)"); return FIN_ENOMEM;
    }
    if (!b->d_total) HIPCHK(hipMalloc((void**)&b->d_total, 8));
    const void* frec = b->last_frec ? b->d_frec : nullptr;
    int rc = fin_launch_sgm_count(frec, (const uint64_t*)b->d_out_offs, b->d_out, nr, b->dev.k, (uint32_t*)b->d_sgm_cnt, (uint32_t*)b->d_sgm_bsum, (uint64_t*)b->d_sgm_boff, b->d_total, st);
    if (rc != 0) { set_err(err, errlen, std::string("segment kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, b->d_total, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (batch_grow(b, &b->d_sgm, b->cap_sgm, (size_t)total * 16 + 16, st)) { set_err(err, errlen, "out of device memory (segments)"); return FIN_ENOMEM; }
    rc = fin_launch_sgm_write(frec, (const uint64_t*)b->d_out_offs, b->d_out, nr, b->dev.k, (const uint32_t*)b->d_sgm_cnt, (const uint64_t*)b->d_sgm_boff, (uint64_t*)b->d_sgm_offs, b->d_sgm, st);
    if (rc != 0) { set_err(err, errlen, std::string("segment kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    b->n_segments = total; b->sgm_ready = true;
    if (n_segments) *n_segments = total;
    return FIN_OK;
}

void* fin_batch_device_segments(const fin_batch* b) { return b && b->sgm_ready ? b->d_sgm : nullptr; }
void* fin_batch_device_segment_offsets(const fin_batch* b) { return b && b->sgm_ready ? b->d_sgm_offs : nullptr; }

int fin_batch_download_segments(fin_batch* b, uint64_t* seg_offs_out, fin_segment* segs_out, char* err, size_t errlen) {
    if (!b || !seg_offs_out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (!b->sgm_ready) { set_err(err, errlen, "fin_batch_segments first"); return FIN_EINVAL; }
    if (b->n_segments && !segs_out) { set_err(err, errlen, "null segment buffer"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    HIPCHK(hipMemcpyAsync(seg_offs_out, b->d_sgm_offs, (size_t)b->n_reads * 8 + 8, hipMemcpyDeviceToHost, st));
    if (b->n_segments) HIPCHK(hipMemcpyAsync(segs_out, b->d_sgm, (size_t)b->n_segments * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FIN_OK;
}

// ---- per-read summaries and the screen made from them (fin_readsum.hip) -------------------------------------------------------------
static_assert(sizeof(fin_read_summary) == 16, "a read summary is 16 bytes");

int fin_batch_read_summaries(fin_batch* b, char* err, size_t errlen) {
    if (!b) { set_err(err, errlen, "null batch"); return FIN_EINVAL; }
    if (!b->ran) { set_err(err, errlen, "this batch has not run: there is nothing to summarise (fin_batch_run first)"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    b->rsum_ready = false; b->scr_ready = false;
    // (no read has a k-mer: the step searched nothing, there is no overflow list to look at -- every summary is zero)
    if (b->n_kmers != 0) if (const int orc = batch_overrun_check(b, st, err, errlen)) return orc;   // a run without results: nothing is written
    const uint32_t nr = (uint32_t)b->n_reads;
    if (batch_grow(b, &b->d_rsum, b->cap_rsum, (size_t)nr * 16 + 16, st)) { set_err(err, errlen, "out of device memory (read summaries)"); return FIN_ENOMEM; }
    if (b->n_kmers == 0) HIPCHK(hipMemsetAsync(b->d_rsum, 0, (size_t)nr * 16 + 16, st));
    else {
        const int rc = fin_launch_read_summaries(b->last_frec ? b->d_frec : nullptr, (const uint64_t*)b->d_out_offs, b->d_out, nr, b->dev.k, b->d_rsum, st);
        if (rc != 0) { set_err(err, errlen, std::string("read summary kernel: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    }
    b->rsum_ready = true;
    return FIN_OK;
}

void* fin_batch_device_read_summaries(const fin_batch* b) { return b && b->rsum_ready ? b->d_rsum : nullptr; }

int fin_batch_download_read_summaries(fin_batch* b, fin_read_summary* out, char* err, size_t errlen) {
    if (!b || (b->n_reads && !out)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (!b->rsum_ready) { set_err(err, errlen, "fin_batch_read_summaries first"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    if (b->n_reads) HIPCHK(hipMemcpyAsync(out, b->d_rsum, (size_t)b->n_reads * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FIN_OK;
}

int fin_batch_screen(fin_batch* b, uint32_t min_found, uint32_t min_permille, int invert, uint64_t* n_pass, char* err, size_t errlen) {
    if (!b) { set_err(err, errlen, "null batch"); return FIN_EINVAL; }
    if (min_permille > 1000u) { set_err(err, errlen, "min_permille is a share in thousandths: 0 .. 1000"); return FIN_EINVAL; }
    if (!b->rsum_ready) if (const int rc = fin_batch_read_summaries(b, err, errlen)) return rc;
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    b->scr_ready = false;
    const uint32_t nr = (uint32_t)b->n_reads, nb = fin_rsm_blocks(nr);
    if (batch_grow(b, &b->d_scr_bits, b->cap_scr_bits, (size_t)((nr + 63u) / 64u) * 8 + 8, st) || batch_grow(b, &b->d_scr_bsum, b->cap_scr_bsum, (size_t)nb * 4 + 4, st) ||
        batch_grow(b, &b->d_scr_boff, b->cap_scr_boff, (size_t)nb * 8 + 8, st)) {
        set_err(err, errlen, "out of device memory (screen tables)"); return FIN_ENOMEM;
    }
    if (!b->d_total) HIPCHK(hipMalloc((void**)&b->d_total, 8));
    int rc = fin_launch_screen_bits(b->d_rsum, (const uint64_t*)b->d_out_offs, nr, min_found, min_permille, invert, (uint64_t*)b->d_scr_bits, (uint32_t*)b->d_scr_bsum,
                                    (uint64_t*)b->d_scr_boff, b->d_total, st);
    if (rc != 0) { set_err(err, errlen, std::string("screen kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, b->d_total, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (total > nr) { set_err(err, errlen, "screen kernels: more passing reads than reads"); return FIN_ENODEV; }
    if (batch_grow(b, &b->d_scr_ids, b->cap_scr_ids, (size_t)total * 4 + 16, st)) { set_err(err, errlen, "out of device memory (screen ids)"); return FIN_ENOMEM; }
    rc = fin_launch_screen_ids((const uint64_t*)b->d_scr_bits, (const uint64_t*)b->d_scr_boff, nr, (uint32_t*)b->d_scr_ids, st);
    if (rc != 0) { set_err(err, errlen, std::string("screen kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    b->n_pass = total; b->scr_ready = true;
    if (n_pass) *n_pass = total;
    return FIN_OK;
}

void* fin_batch_device_screen_ids(const fin_batch* b) { return b && b->scr_ready ? b->d_scr_ids : nullptr; }
void* fin_batch_device_screen_bits(const fin_batch* b) { return b && b->scr_ready ? b->d_scr_bits : nullptr; }

int fin_batch_download_screen(fin_batch* b, uint32_t* ids_out, uint64_t* bits_out, char* err, size_t errlen) {
    if (!b) { set_err(err, errlen, "null batch"); return FIN_EINVAL; }
    if (!b->scr_ready) { set_err(err, errlen, "fin_batch_screen first"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    const size_t n_words = (size_t)((b->n_reads + 63) / 64);
    if (ids_out && b->n_pass) HIPCHK(hipMemcpyAsync(ids_out, b->d_scr_ids, (size_t)b->n_pass * 4, hipMemcpyDeviceToHost, st));
    if (bits_out && n_words) HIPCHK(hipMemcpyAsync(bits_out, b->d_scr_bits, n_words * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FIN_OK;
}

// ---- the profile over the unitig set (fin_hits.hip) ---------------------------------------------------------------------------------
// what the download of a device accumulator (fin_hits, fin_cover, fin_depth, fin_pileup) waits for: an event per stream that work on the accumulator was put on
extern "C++" {   // (templates among them)
struct AccPending {
    std::mutex mu; std::vector<std::pair<hipStream_t, hipEvent_t>> pending;
    int mark(hipStream_t st, char* err, size_t errlen) {
        std::lock_guard<std::mutex> g(mu);
        return mark_locked(st, err, errlen);
    }
    int wait(char* err, size_t errlen) {
        std::lock_guard<std::mutex> g(mu);
        for (auto& p : pending) HIPCHK(hipEventSynchronize(p.second));
        return FIN_OK;
    }
    // `st` waits for everything marked so far (a reader of the accumulator on another stream than its adds)
    int order(hipStream_t st, char* err, size_t errlen) {
        std::lock_guard<std::mutex> g(mu);
        return order_locked(st, err, errlen);
    }
    // a reset does not commute with the adds: it runs behind everything issued so far on other streams, and every later add on another stream runs behind it
    // (the reset's own event -- a stream's mark is recorded again by its next add --, which behind_reset makes an add's stream wait for).  One lock is held from
    // the waits over the zeroing (a memset of `bytes` at `p`, on `st`) to the two records, so an add from another host thread falls before the reset or behind it,
    // never in between.  Adds among themselves stay unordered: they are atomic and commute
    hipStream_t reset_st = nullptr; hipEvent_t reset_ev = nullptr;
    int reset(hipStream_t st, void* p, size_t bytes) {
        char* err = nullptr; const size_t errlen = 0;
        std::lock_guard<std::mutex> g(mu);
        if (const int orc = order_locked(st, err, errlen)) return orc;
        if (hipMemsetAsync(p, 0, bytes, st) != hipSuccess) return FIN_ENODEV;
        if (!reset_ev) HIPCHK(hipEventCreateWithFlags(&reset_ev, hipEventDisableTiming));
        HIPCHK(hipEventRecord(reset_ev, st));
        reset_st = st;
        return mark_locked(st, err, errlen);
    }
    // a change of the accumulator's FORM (fin_colors_compact, fin_colors_expand) is ordered as a reset is: f() puts its work on `st` behind everything issued so
    // far, with the one lock held from the waits to the two records; every later add on another stream runs behind it.  f() failed: nothing is recorded
    template <class F> int reform(hipStream_t st, F&& f, char* err, size_t errlen) {
        std::lock_guard<std::mutex> g(mu);
        if (const int orc = order_locked(st, err, errlen)) return orc;
        if (const int frc = f()) return frc;
        if (!reset_ev) HIPCHK(hipEventCreateWithFlags(&reset_ev, hipEventDisableTiming));
        HIPCHK(hipEventRecord(reset_ev, st));
        reset_st = st;
        return mark_locked(st, err, errlen);
    }
    int behind_reset(hipStream_t st, char* err, size_t errlen) {
        std::lock_guard<std::mutex> g(mu);
        if (reset_ev && reset_st != st) HIPCHK(hipStreamWaitEvent(st, reset_ev, 0));
        return FIN_OK;
    }
    void drop() {
        for (auto& p : pending) { (void)hipEventSynchronize(p.second); (void)hipEventDestroy(p.second); }
        pending.clear();
        if (reset_ev) { (void)hipEventSynchronize(reset_ev); (void)hipEventDestroy(reset_ev); reset_ev = nullptr; }
    }
private:   // (with `mu` held)
    int mark_locked(hipStream_t st, char* err, size_t errlen) {
        for (auto& p : pending) if (p.first == st) { HIPCHK(hipEventRecord(p.second, st)); return FIN_OK; }
        hipEvent_t ev = nullptr;
        HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        pending.push_back({st, ev});
        HIPCHK(hipEventRecord(ev, st));
        return FIN_OK;
    }
    int order_locked(hipStream_t st, char* err, size_t errlen) {
        for (auto& p : pending) if (p.first != st) HIPCHK(hipStreamWaitEvent(st, p.second, 0));
        return FIN_OK;
    }
};
// what the seven device accumulators are alike in (they are opaque in finito_amd.h): the index and device they live beside, and what their readers wait for
struct fin_acc {
    const fin_index* idx = nullptr;
    int device = -1;
    AccPending pend;
};
// ---- the accumulators' frame: each step of create / free / reset / download / add that they share, stated once --------------------------------------------
// create, behind the caller's own argument checks: the replica the accumulator goes beside (`rep`, may be null, learns it), the device made current
static int acc_create_open(const fin_index* idx, int device, const fin_index::Replica** rep, char* err, size_t errlen) {
    const fin_index::Replica* r = idx->replica_on(device);
    if (!r) { set_err(err, errlen, "index is not resident on that device: call fin_index_to_device first (no CPU fallback)"); return FIN_ENODEV; }
    if (idx->n_unitigs >= 0x80000000ull) { set_err(err, errlen, "more than 2^31-1 unitigs"); return FIN_ELIMIT; }
    HIPCHK(hipSetDevice(device));
    if (rep) *rep = r;
    return FIN_OK;
}
template <class A> static A* acc_new(const fin_index* idx, int device, char* err, size_t errlen) {
    A* a = new (std::nothrow) A();
    if (!a) { set_err(err, errlen, "out of memory"); return nullptr; }
    a->idx = idx; a->device = device;
    return a;
}
// the accumulator's buffer of `bytes`, its first `zero_bytes` zeroed.  The two unwinds: a failed allocation deletes the bare struct, a failed memset goes through
// the accumulator's own free (`no_room` is the whole message of the first)
template <class A> static int acc_alloc_zero(A* a, void** p, size_t bytes, size_t zero_bytes, const char* no_room, void (*free_a)(A*), char* err, size_t errlen) {
    if (hipMalloc(p, bytes) != hipSuccess) { (void)hipGetLastError(); delete a; set_err(err, errlen, no_room); return FIN_ENOMEM; }
    if (hipMemset(*p, 0, zero_bytes) != hipSuccess) { free_a(a); set_err(err, errlen, "hipMemset failed"); return FIN_ENODEV; }
    return FIN_OK;
}
// free: false for null; else the device is current and nothing is pending any more -- the caller frees its buffers and deletes
static bool acc_free_open(fin_acc* a) {
    if (!a) return false;
    if (a->device >= 0) (void)hipSetDevice(a->device);
    a->pend.drop();
    return true;
}
static int acc_reset(fin_acc* a, void* hip_stream, void* p, size_t bytes) {
    if (!a) return FIN_EINVAL;
    if (hipSetDevice(a->device) != hipSuccess) return FIN_ENODEV;
    return a->pend.reset((hipStream_t)hip_stream, p, bytes);
}
// download: the device current, the adds waited for, and the flag word at `d_flags` (null: the accumulator has none) read -- flag 1 answers FIN_ELIMIT with
// `flag1`, flag 2 FIN_EINVAL with `flag2` (null: no such flag)
static int acc_download_open(fin_acc* a, const uint32_t* d_flags, const char* flag1, const char* flag2, char* err, size_t errlen) {
    HIPCHK(hipSetDevice(a->device));
    if (const int wrc = a->pend.wait(err, errlen)) return wrc;
    if (!d_flags) return FIN_OK;
    uint32_t flags = 0;
    HIPCHK(hipMemcpy(&flags, d_flags, 4, hipMemcpyDeviceToHost));
    if (flags & 1u) { set_err(err, errlen, flag1); return FIN_ELIMIT; }
    if (flag2 && (flags & 2u)) { set_err(err, errlen, flag2); return FIN_EINVAL; }
    return FIN_OK;
}
// where a download's numbers go when the caller wants only their sum: `dst`, or a temporary of n entries
template <class T> static T* dst_or_tmp(T* dst, std::vector<T>& tmp, size_t n) {
    if (!dst) { tmp.resize(n); dst = tmp.data(); }
    return dst;
}
template <class T, class F> static uint64_t sum_of(const T* v, size_t n, F what) {
    uint64_t t = 0;
    for (size_t q = 0; q < n; q++) t += (uint64_t)what(v[q]);
    return t;
}
// `st` waits for what was put on `src` so far (rows or classes made on the run's stream, behind the run, and added on another)
static int stream_behind(hipStream_t st, hipStream_t src, char* err, size_t errlen) {
    if (st == src) return FIN_OK;
    hipEvent_t ev = nullptr;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, src);
    if (e == hipSuccess) e = hipStreamWaitEvent(st, ev, 0);
    (void)hipEventDestroy(ev);   // (released once it has completed)
    HIPCHK(e);
    return FIN_OK;
}
// behind the batch's most recent run, whichever stream it was launched on: what every fin_batch_add_* checks and orders alike
static int acc_behind_run(fin_batch* b, const fin_index* acc_idx, int acc_device, hipStream_t st, char* err, size_t errlen) {
    if (!b->ran) { set_err(err, errlen, "this batch has not run: there are no hits to add (fin_batch_run first)"); return FIN_EINVAL; }
    if (b->idx != acc_idx || b->device != acc_device) { set_err(err, errlen, "batch and accumulator belong to different indexes or devices"); return FIN_EINVAL; }
    if (b->ovf_state == 2) { set_err(err, errlen, "the overflow list of this batch overran: results withheld"); return FIN_ELIMIT; }
    HIPCHK(hipSetDevice(b->device));
    if (st != b->last_stream) {
        hipEvent_t ev = b->runs.back().e[4];
        HIPCHK(hipStreamWaitEvent(st, ev, 0));
    }
    return FIN_OK;
}
// the frame of an add: behind the run and behind the accumulator's last reset; then the caller launches on `st`, and acc_add_close turns the launch's result
// into the message `what` + the error's name, or marks `st` for the downloads
static int acc_add_open(fin_batch* b, fin_acc* a, hipStream_t st, char* err, size_t errlen) {
    if (const int brc = acc_behind_run(b, a->idx, a->device, st, err, errlen)) return brc;
    return a->pend.behind_reset(st, err, errlen);
}
static int acc_add_close(fin_acc* a, hipStream_t st, int launch_rc, const char* what, char* err, size_t errlen) {
    if (launch_rc != 0) { set_err(err, errlen, std::string(what) + hipGetErrorString((hipError_t)launch_rc)); return FIN_ENODEV; }
    return a->pend.mark(st, err, errlen);
}
// the argument tests that several entry points make, each with its message
static const char* const BAD_PERMILLE = "permille is a share in thousandths: 0 .. 1000";
static const char* const BAD_MIN_PERMILLE = "min_permille is a share in thousandths: 0 .. 1000";
static int check_permille(uint32_t permille, const char* bad, char* err, size_t errlen) {
    if (permille > 1000u) { set_err(err, errlen, bad); return FIN_EINVAL; }
    return FIN_OK;
}
static int check_pair_mode(uint32_t mode, char* err, size_t errlen) {
    if (mode != FIN_PAIR_ANY && mode != FIN_PAIR_BOTH) { set_err(err, errlen, "mode is FIN_PAIR_ANY (0) or FIN_PAIR_BOTH (1)"); return FIN_EINVAL; }
    return FIN_OK;
}
static int check_even(uint64_t n_reads, char* err, size_t errlen) {
    if (n_reads & 1u) { set_err(err, errlen, "paired pseudoalignment wants interleaved mates: " + std::to_string(n_reads) + " reads are an odd number"); return FIN_EINVAL; }
    return FIN_OK;
}
}  // extern "C++"

struct fin_hits : fin_acc {
    uint64_t n_unitigs = 0;
    void* d_counts = nullptr;   // uint64[n_unitigs], then the flag word (fin_launch_hits_add)
};
static uint32_t* hits_flags(const fin_hits* h) { return (uint32_t*)((uint64_t*)h->d_counts + h->n_unitigs); }

void fin_hits_free(fin_hits* h) {
    if (!acc_free_open(h)) return;
    (void)hipFree(h->d_counts);
    delete h;
}

int fin_hits_create(const fin_index* idx, int device, fin_hits** out, char* err, size_t errlen) {
    if (!idx || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    *out = nullptr;
    if (const int orc = acc_create_open(idx, device, nullptr, err, errlen)) return orc;
    fin_hits* h = acc_new<fin_hits>(idx, device, err, errlen);
    if (!h) return FIN_ENOMEM;
    h->n_unitigs = idx->n_unitigs;
    if (const int arc = acc_alloc_zero(h, &h->d_counts, h->n_unitigs * 8 + 8, h->n_unitigs * 8 + 8, "out of device memory (unitig counts)", fin_hits_free, err, errlen)) return arc;
    *out = h;
    return FIN_OK;
}

int fin_hits_reset(fin_hits* h, void* hip_stream) {
    return acc_reset(h, hip_stream, h ? h->d_counts : nullptr, h ? h->n_unitigs * 8 + 8 : 0);
}

void* fin_hits_device_counts(const fin_hits* h) { return h ? h->d_counts : nullptr; }

int fin_batch_add_hits(fin_batch* b, fin_hits* h, void* hip_stream, char* err, size_t errlen) {
    if (!b || !h) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    hipStream_t st = (hipStream_t)hip_stream;
    if (const int orc = acc_add_open(b, h, st, err, errlen)) return orc;
    const int rc = fin_launch_hits_add(b->last_frec ? b->d_frec : nullptr, (const uint64_t*)b->d_out_offs, b->d_out, (uint32_t)b->n_reads, b->n_kmers, b->dev.k, h->d_counts,
                                       (uint32_t)h->n_unitigs, hits_flags(h), b->d_ovf_count, b->last_ovf_cap, (uint32_t)optv(b->idx, O_hits_combine), st);
    return acc_add_close(h, st, rc, "hits kernel: ", err, errlen);
}

int fin_hits_download(fin_hits* h, uint64_t* counts_out, uint64_t* total, char* err, size_t errlen) {
    if (!h || (h->n_unitigs && !counts_out && !total)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int orc = acc_download_open(h, hits_flags(h), "a step whose overflow list overran was added: it has no results, nothing of it was counted (reset the accumulator)",
                                          "a pair with a unitig number outside the index was met (not counted)", err, errlen)) return orc;
    std::vector<uint64_t> tmp;
    uint64_t* const dst = dst_or_tmp(counts_out, tmp, (size_t)h->n_unitigs);
    if (h->n_unitigs) HIPCHK(hipMemcpy(dst, h->d_counts, h->n_unitigs * 8, hipMemcpyDeviceToHost));
    if (total) *total = sum_of(dst, (size_t)h->n_unitigs, [](uint64_t v) { return v; });
    return FIN_OK;
}

// ---- read classification by unitig labels (fin_classify.hip) ---------------------------------------------------------------------------
static_assert(sizeof(fin_read_class) == 16, "a read class is 16 bytes");
struct fin_labels : fin_acc {
    uint64_t n_unitigs = 0; uint32_t n_labels = 0;
    uint64_t serial = 0;        // which labelling a batch's classes were made for (an address can come back after a free)
    void* d_labels = nullptr;   // uint32[n_unitigs]
    void* d_reads = nullptr;    // the tally: uint64[n_labels + 1]
};
static std::atomic<uint64_t> g_labels_serial{0};

void fin_labels_free(fin_labels* l) {
    if (!acc_free_open(l)) return;
    (void)hipFree(l->d_labels); (void)hipFree(l->d_reads);
    delete l;
}

int fin_labels_create(const fin_index* idx, int device, const uint32_t* unitig_labels, uint32_t n_labels, fin_labels** out, char* err, size_t errlen) {
    if (!idx || !out || (idx->n_unitigs && !unitig_labels)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    *out = nullptr;
    if (n_labels == 0 || n_labels > 0x80000000u) { set_err(err, errlen, "n_labels is 1 .. 2^31"); return FIN_EINVAL; }
    for (uint64_t u = 0; u < idx->n_unitigs; u++)
        if (unitig_labels[u] != FIN_NO_LABEL && unitig_labels[u] >= n_labels) {
            set_err(err, errlen, "unitig " + std::to_string(u) + " has label " + std::to_string(unitig_labels[u]) + ": neither below n_labels = " + std::to_string(n_labels) + " nor FIN_NO_LABEL");
            return FIN_EINVAL;
        }
    if (const int orc = acc_create_open(idx, device, nullptr, err, errlen)) return orc;
    fin_labels* l = acc_new<fin_labels>(idx, device, err, errlen);
    if (!l) return FIN_ENOMEM;
    l->n_unitigs = idx->n_unitigs; l->n_labels = n_labels; l->serial = ++g_labels_serial;
    const size_t tally = ((size_t)n_labels + 1) * 8;
    if (hipMalloc(&l->d_labels, (size_t)l->n_unitigs * 4 + 16) != hipSuccess || hipMalloc(&l->d_reads, tally) != hipSuccess) {
        (void)hipGetLastError(); fin_labels_free(l); set_err(err, errlen, "out of device memory (unitig labels and tally)"); return FIN_ENOMEM;
    }
    if ((l->n_unitigs && hipMemcpy(l->d_labels, unitig_labels, (size_t)l->n_unitigs * 4, hipMemcpyHostToDevice) != hipSuccess) || hipMemset(l->d_reads, 0, tally) != hipSuccess) {
        fin_labels_free(l); set_err(err, errlen, "copying the labels failed"); return FIN_ENODEV;
    }
    *out = l;
    return FIN_OK;
}

int fin_labels_reset(fin_labels* l, void* hip_stream) {
    return acc_reset(l, hip_stream, l ? l->d_reads : nullptr, l ? ((size_t)l->n_labels + 1) * 8 : 0);
}

void* fin_labels_device_labels(const fin_labels* l) { return l ? l->d_labels : nullptr; }
void* fin_labels_device_reads(const fin_labels* l) { return l ? l->d_reads : nullptr; }

int fin_labels_download(fin_labels* l, uint64_t* reads_out, uint64_t* total, char* err, size_t errlen) {
    if (!l) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int orc = acc_download_open(l, nullptr, nullptr, nullptr, err, errlen)) return orc;   // (a tally has no flags)
    if (!reads_out && !total) return FIN_OK;
    const size_t n = (size_t)l->n_labels + 1;
    std::vector<uint64_t> tmp;
    uint64_t* const dst = dst_or_tmp(reads_out, tmp, n);
    HIPCHK(hipMemcpy(dst, l->d_reads, n * 8, hipMemcpyDeviceToHost));
    if (total) *total = sum_of(dst, n, [](uint64_t v) { return v; });
    return FIN_OK;
}

int fin_batch_classify(fin_batch* b, const fin_labels* l, char* err, size_t errlen) {
    if (!b || !l) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (!b->ran) { set_err(err, errlen, "this batch has not run: there is nothing to classify (fin_batch_run first)"); return FIN_EINVAL; }
    if (b->idx != l->idx || b->device != l->device) { set_err(err, errlen, "batch and labelling belong to different indexes or devices"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    b->cls_ready = false;
    // (no read has a k-mer: the step searched nothing, there is no overflow list to look at -- every class is the empty one)
    if (b->n_kmers != 0) if (const int orc = batch_overrun_check(b, st, err, errlen)) return orc;   // a run without results: nothing is written
    const uint32_t nr = (uint32_t)b->n_reads;
    if (batch_grow(b, &b->d_cls, b->cap_cls, (size_t)nr * 16 + 16, st)) { set_err(err, errlen, "out of device memory (read classes)"); return FIN_ENOMEM; }
    const int rc = fin_launch_classify(b->n_kmers != 0 && b->last_frec ? b->d_frec : nullptr, (const uint64_t*)b->d_out_offs, b->d_out, nr, b->dev.k,
                                       (const uint32_t*)l->d_labels, (uint32_t)l->n_unitigs, b->d_cls, st);
    if (rc != 0) { set_err(err, errlen, std::string("classify kernel: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    b->cls_ready = true; b->cls_labels = l->serial;
    return FIN_OK;
}

void* fin_batch_device_read_classes(const fin_batch* b) { return b && b->cls_ready ? b->d_cls : nullptr; }

int fin_batch_download_read_classes(fin_batch* b, fin_read_class* out, char* err, size_t errlen) {
    if (!b || (b->n_reads && !out)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (!b->cls_ready) { set_err(err, errlen, "fin_batch_classify first"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    if (b->n_reads) HIPCHK(hipMemcpyAsync(out, b->d_cls, (size_t)b->n_reads * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FIN_OK;
}

int fin_batch_add_classes(fin_batch* b, fin_labels* l, uint32_t min_found, uint32_t min_permille, uint32_t min_margin, void* hip_stream, char* err, size_t errlen) {
    if (!b || !l) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int crc = check_permille(min_permille, BAD_MIN_PERMILLE, err, errlen)) return crc;
    if (!b->cls_ready || b->cls_labels != l->serial) if (const int rc = fin_batch_classify(b, l, err, errlen)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (const int orc = acc_add_open(b, l, st, err, errlen)) return orc;
    if (const int src = stream_behind(st, b->last_stream, err, errlen)) return src;   // the classes were made on the run's stream, behind the run: the add waits for them too
    const int rc = fin_launch_class_tally(b->d_cls, (const uint64_t*)b->d_out_offs, (uint32_t)b->n_reads, l->n_labels, min_found, min_permille, min_margin,
                                          (uint64_t*)l->d_reads, st);
    return acc_add_close(l, st, rc, "class tally kernel: ", err, errlen);
}

// ---- colour sets per unitig and read pseudoalignment (fin_colors.hip) -------------------------------------------------------------------
static_assert(sizeof(fin_read_pseudo) == 16, "a pseudoalignment head is 16 bytes");
struct fin_colors : fin_acc {
    uint64_t n_unitigs = 0; uint32_t n_colors = 0, words = 0;
    void* d_bits = nullptr;     // DENSE: uint64[n_unitigs * words], then the flag word (fin_launch_colors_add); null while compact
    // COMPACT (fin_colorsets.hip; fin_colors_compact, fin_colors_upload_sets): these two in place of d_bits.  A compact object has no flags: a flagged matrix is not compacted
    bool compact = false; uint64_t n_sets = 0;
    void* d_set_of = nullptr;   // uint32[n_unitigs]
    void* d_sets = nullptr;     // uint64[(n_sets + 1) * words], row 0 zero
    uint64_t cs_stats[4] = {0, 0, 0, 0};   // fin_colors_compact_stats
    // fin_colors_coverage's: made by the first call, kept
    void* d_ccv = nullptr;      // uint64[(n_colors + 1) * 8]: the table and the uncoloured entry; then the class byte of every unitig
    std::mutex ccv_mu;          // one projection at a time goes through d_ccv
    // fin_colors_depth_histogram's: made by the first call, grown when a later one asks for more, kept (as d_ccv is: hipFree would synchronise the device in every call)
    void* d_dh = nullptr;       // the table uint64[n_colors][2][n_bins] and the uncoloured histogram behind it; 64 bytes of the class kernel's scratch; the class bytes; the sub-range's uint32[unitigs][n_bins]
    size_t dh_bytes = 0;
    std::mutex dh_mu;           // one call at a time goes through d_dh
};
static size_t colors_bytes(const fin_colors* c) { return (size_t)c->n_unitigs * c->words * 8; }
static uint32_t* colors_flags(const fin_colors* c) { return (uint32_t*)((char*)c->d_bits + colors_bytes(c)); }

void fin_colors_free(fin_colors* c) {
    if (!acc_free_open(c)) return;
    (void)hipFree(c->d_bits); (void)hipFree(c->d_ccv); (void)hipFree(c->d_dh); (void)hipFree(c->d_set_of); (void)hipFree(c->d_sets);
    delete c;
}

int fin_colors_create(const fin_index* idx, int device, uint32_t n_colors, fin_colors** out, char* err, size_t errlen) {
    if (!idx || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    *out = nullptr;
    if (n_colors == 0 || n_colors > FIN_MAX_COLORS) { set_err(err, errlen, "n_colors is 1 .. " + std::to_string(FIN_MAX_COLORS)); return FIN_ELIMIT; }
    if (const int orc = acc_create_open(idx, device, nullptr, err, errlen)) return orc;
    fin_colors* c = acc_new<fin_colors>(idx, device, err, errlen);
    if (!c) return FIN_ENOMEM;
    c->n_unitigs = idx->n_unitigs; c->n_colors = n_colors; c->words = (n_colors + 63u) / 64u;
    if (const int arc = acc_alloc_zero(c, &c->d_bits, colors_bytes(c) + 8, colors_bytes(c) + 8, "out of device memory (colour matrix)", fin_colors_free, err, errlen)) return arc;
    *out = c;
    return FIN_OK;
}

// the two forms of a fin_colors (finito_amd.h, "DEDUPLICATED COLOUR SETS").  What reads bits[u * W + w] directly refuses a compact object with this message
static const char* const COLORS_COMPACT = "the colours are compact (deduplicated sets): fin_colors_expand first";
static int colors_want_dense(const fin_colors* c, char* err, size_t errlen) {
    if (!c->compact) return FIN_OK;
    set_err(err, errlen, COLORS_COMPACT);
    return FIN_EINVAL;
}
// a compact object gets an (unwritten) dense matrix in place of its sets: what fin_colors_upload and fin_colors_reset then fill.  The device is current; the sets
// are freed once the device has finished whatever still reads them
static int colors_make_dense(fin_colors* c, char* err, size_t errlen) {
    if (!c->compact) return FIN_OK;
    void* bits = nullptr;
    if (hipMalloc(&bits, colors_bytes(c) + 8) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "out of device memory (colour matrix)"); return FIN_ENOMEM; }
    (void)hipDeviceSynchronize();
    (void)hipFree(c->d_set_of); (void)hipFree(c->d_sets);
    c->d_set_of = c->d_sets = nullptr; c->d_bits = bits; c->compact = false; c->n_sets = 0;
    for (uint64_t& v : c->cs_stats) v = 0;  // (they describe the compact form that goes)
    return FIN_OK;
}

int fin_colors_upload(fin_colors* c, const uint64_t* bits, char* err, size_t errlen) {
    if (!c || (c->n_unitigs && !bits)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    const uint64_t bad = colors_first_stray(bits, c->n_unitigs, c->n_colors, c->words);
    if (bad != c->n_unitigs) { set_err(err, errlen, "unitig " + std::to_string(bad) + " has a bit at or above n_colors = " + std::to_string(c->n_colors) + " set"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (const int wrc = c->pend.wait(err, errlen)) return wrc;
    if (const int drc = colors_make_dense(c, err, errlen)) return drc;
    if (c->n_unitigs) HIPCHK(hipMemcpy(c->d_bits, bits, colors_bytes(c), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(colors_flags(c), 0, 8));
    return FIN_OK;
}

int fin_colors_reset(fin_colors* c, void* hip_stream) {
    if (c && c->compact) {
        if (hipSetDevice(c->device) != hipSuccess) return FIN_ENODEV;
        if (const int drc = colors_make_dense(c, nullptr, 0)) return drc;
    }
    return acc_reset(c, hip_stream, c ? c->d_bits : nullptr, c ? colors_bytes(c) + 8 : 0);
}

void* fin_colors_device_bits(const fin_colors* c) { return c && !c->compact ? c->d_bits : nullptr; }
uint32_t fin_colors_n_colors(const fin_colors* c) { return c ? c->n_colors : 0; }
uint32_t fin_colors_words(const fin_colors* c) { return c ? c->words : 0; }

// the sets of a compact object on the host (the device current, the object's work waited for)
static int colors_sets_to_host(fin_colors* c, std::vector<uint32_t>& set_of, std::vector<uint64_t>& sets, char* err, size_t errlen) {
    set_of.resize((size_t)c->n_unitigs); sets.resize((size_t)(c->n_sets + 1) * c->words);
    if (c->n_unitigs) HIPCHK(hipMemcpy(set_of.data(), c->d_set_of, (size_t)c->n_unitigs * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sets.data(), c->d_sets, sets.size() * 8, hipMemcpyDeviceToHost));
    return FIN_OK;
}
// fin_colors_download of a compact object: the dense matrix expanded on the host, the set bits counted per set; the object stays compact
static int colors_download_compact(fin_colors* c, uint64_t* bits_out, uint64_t* n_set, char* err, size_t errlen) {
    if (const int orc = acc_download_open(c, nullptr, nullptr, nullptr, err, errlen)) return orc;   // (a compact object has no flags)
    if (!bits_out && !n_set) return FIN_OK;
    std::vector<uint32_t> set_of; std::vector<uint64_t> sets;
    if (const int rc = colors_sets_to_host(c, set_of, sets, err, errlen)) return rc;
    const uint32_t W = c->words;
    if (bits_out) for (size_t u = 0; u < set_of.size(); u++) memcpy(bits_out + u * W, sets.data() + (size_t)set_of[u] * W, (size_t)W * 8);
    if (n_set) {
        std::vector<uint32_t> pc((size_t)c->n_sets + 1, 0);
        for (size_t q = 0; q < pc.size(); q++) pc[q] = (uint32_t)sum_of(sets.data() + q * W, W, [](uint64_t w) { return __builtin_popcountll(w); });
        *n_set = sum_of(set_of.data(), set_of.size(), [&](uint32_t q) { return pc[q]; });
    }
    return FIN_OK;
}

int fin_colors_download(fin_colors* c, uint64_t* bits_out, uint64_t* n_set, char* err, size_t errlen) {
    if (!c) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (c->compact) return colors_download_compact(c, bits_out, n_set, err, errlen);
    if (const int orc = acc_download_open(c, colors_flags(c), "a step whose overflow list overran was added: it has no results, nothing of it was coloured (reset the colours)",
                                          nullptr, err, errlen)) return orc;
    if (!bits_out && !n_set) return FIN_OK;
    const size_t n = (size_t)c->n_unitigs * c->words;
    std::vector<uint64_t> tmp;
    uint64_t* const dst = dst_or_tmp(bits_out, tmp, n);
    if (n) HIPCHK(hipMemcpy(dst, c->d_bits, n * 8, hipMemcpyDeviceToHost));
    if (n_set) *n_set = sum_of(dst, n, [](uint64_t w) { return __builtin_popcountll(w); });
    return FIN_OK;
}

// ---- the compact state: deduplicated colour sets (fin_colorsets.hip) ----
int fin_colors_is_compact(const fin_colors* c) { return c && c->compact ? 1 : 0; }
uint64_t fin_colors_n_sets(const fin_colors* c) { return c && c->compact ? c->n_sets : 0; }
void* fin_colors_device_set_of(const fin_colors* c) { return c && c->compact ? c->d_set_of : nullptr; }
void* fin_colors_device_sets(const fin_colors* c) { return c && c->compact ? c->d_sets : nullptr; }
int fin_colors_compact_stats(const fin_colors* c, uint64_t out[4]) {
    if (!c || !out) return FIN_EINVAL;
    for (int q = 0; q < 4; q++) out[q] = c->cs_stats[q];
    return FIN_OK;
}

int fin_colors_compact(fin_colors* c, uint64_t max_sets, void* hip_stream, char* err, size_t errlen) {
    if (!c) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (max_sets > (1ull << 26)) { set_err(err, errlen, "max_sets is at most 2^26 (0: the number of unitigs, at most 2^26)"); return FIN_ELIMIT; }
    if (max_sets == 0) max_sets = std::min<uint64_t>(c->n_unitigs, 1ull << 26);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    uint32_t lg = 1;
    while ((1ull << lg) < 2 * max_sets) lg++;
    // (n_unitigs, words and the index are fixed at creation: what is computed here does not depend on the object's form)
    const uint32_t n = (uint32_t)c->n_unitigs, W = c->words, tag_bits = (uint32_t)optv(c->idx, O_colorsets_tag_bits);
    const size_t n_slots = (size_t)1 << lg, nsb = fin_cs_blocks((uint32_t)n_slots);
    // the scratch, sized from n_unitigs and max_sets alone: slots u64 | ctr 4 u64, total | blk_off u64 | slot_of u32 (padded) | slot_id u32 | blk_sum u32
    const size_t o_ctr = n_slots * 8, o_off = o_ctr + 5 * 8, o_slot_of = o_off + nsb * 8, o_slot_id = o_slot_of + (((size_t)n + 1) & ~(size_t)1) * 4, o_sum = o_slot_id + n_slots * 4,
                 tmp_bytes = o_sum + nsb * 4 + 16;
    return c->pend.reform(st, [&]() -> int {
        if (c->compact) return FIN_OK;      // the form is looked at with the object's lock held
        uint32_t flags = 0;
        HIPCHK(hipMemcpyAsync(&flags, colors_flags(c), 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (flags & 1u) { set_err(err, errlen, "a step whose overflow list overran was added: the matrix is not compacted (reset the colours)"); return FIN_ELIMIT; }
        char* tmp = nullptr;
        if (hipMalloc((void**)&tmp, tmp_bytes) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "out of device memory (colour set table)"); return FIN_ENOMEM; }
        void* d_sets = nullptr; void* d_set_of = nullptr;
        uint64_t ctr[5] = {0, 0, 0, 0, 0};
        auto fail = [&](int code, const std::string& msg) { (void)hipStreamSynchronize(st); (void)hipFree(tmp); (void)hipFree(d_sets); (void)hipFree(d_set_of); set_err(err, errlen, msg); return code; };
        if (hipMemsetAsync(tmp, 0, o_off, st) != hipSuccess) return fail(FIN_ENODEV, "hipMemsetAsync failed");
        int rc = fin_launch_cs_claim(c->d_bits, n, W, tmp, lg, tag_bits, max_sets, (uint32_t*)(tmp + o_slot_of), tmp + o_ctr, (uint32_t*)(tmp + o_sum), (uint64_t*)(tmp + o_off),
                                     (uint64_t*)(tmp + o_ctr) + 4, st);
        if (rc != 0) return fail(FIN_ENODEV, std::string("colour set kernels: ") + hipGetErrorString((hipError_t)rc));
        if (hipMemcpyAsync(ctr, tmp + o_ctr, sizeof ctr, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(FIN_ENODEV, "reading the colour set counters failed");
        if ((ctr[3] & 1u) || ctr[4] > max_sets)
            return fail(FIN_ELIMIT, "more than max_sets = " + std::to_string(max_sets) + " distinct non-empty colour rows: the matrix stays dense");
        const uint64_t n_sets = ctr[4];
        if (hipMalloc(&d_sets, (size_t)(n_sets + 1) * W * 8) != hipSuccess || hipMalloc(&d_set_of, (size_t)n * 4 + 16) != hipSuccess) {
            (void)hipGetLastError(); return fail(FIN_ENOMEM, "out of device memory (colour sets)");
        }
        rc = fin_launch_cs_gather(c->d_bits, n, W, tmp, lg, (const uint32_t*)(tmp + o_slot_of), (const uint64_t*)(tmp + o_off), (uint32_t*)(tmp + o_slot_id), d_sets,
                                  (uint32_t*)d_set_of, st);
        if (rc != 0) return fail(FIN_ENODEV, std::string("colour set kernels: ") + hipGetErrorString((hipError_t)rc));
        if (hipDeviceSynchronize() != hipSuccess) return fail(FIN_ENODEV, "the colour set kernels failed");   // (and nothing reads the dense matrix any more)
        (void)hipFree(tmp); (void)hipFree(c->d_bits);
        c->d_bits = nullptr; c->d_sets = d_sets; c->d_set_of = d_set_of; c->n_sets = n_sets; c->compact = true;
        c->cs_stats[0] = n_sets; c->cs_stats[1] = ctr[1]; c->cs_stats[2] = ctr[2]; c->cs_stats[3] = n_slots;
        return FIN_OK;
    }, err, errlen);
}

int fin_colors_expand(fin_colors* c, void* hip_stream, char* err, size_t errlen) {
    if (!c) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    return c->pend.reform(st, [&]() -> int {
        if (!c->compact) return FIN_OK;     // the form is looked at with the object's lock held
        void* bits = nullptr;
        if (hipMalloc(&bits, colors_bytes(c) + 8) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "out of device memory (colour matrix)"); return FIN_ENOMEM; }
        const int rc = fin_launch_cs_expand((const uint32_t*)c->d_set_of, c->d_sets, (uint32_t)c->n_unitigs, c->words, bits, st);
        if (rc != 0 || hipMemsetAsync((char*)bits + colors_bytes(c), 0, 8, st) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            (void)hipFree(bits); set_err(err, errlen, "colour set expand kernel failed"); return FIN_ENODEV;
        }
        (void)hipFree(c->d_set_of); (void)hipFree(c->d_sets);
        c->d_set_of = c->d_sets = nullptr; c->d_bits = bits; c->compact = false; c->n_sets = 0;
        for (uint64_t& v : c->cs_stats) v = 0;
        return FIN_OK;
    }, err, errlen);
}

int fin_colors_download_sets(fin_colors* c, uint32_t* set_of_out, uint64_t* sets_out, uint64_t cap_sets, uint64_t* n_sets, char* err, size_t errlen) {
    if (n_sets) *n_sets = c && c->compact ? c->n_sets : 0;
    if (!c || !n_sets) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (!c->compact) { set_err(err, errlen, "the colours are dense: fin_colors_compact or fin_colors_upload_sets first"); return FIN_EINVAL; }
    if (const int orc = acc_download_open(c, nullptr, nullptr, nullptr, err, errlen)) return orc;
    if (cap_sets < c->n_sets + 1) { set_err(err, errlen, "room for " + std::to_string(cap_sets) + " rows, the sets are " + std::to_string(c->n_sets) + " + the empty one"); return FIN_ELIMIT; }
    if (set_of_out && c->n_unitigs) HIPCHK(hipMemcpy(set_of_out, c->d_set_of, (size_t)c->n_unitigs * 4, hipMemcpyDeviceToHost));
    if (sets_out) HIPCHK(hipMemcpy(sets_out, c->d_sets, (size_t)(c->n_sets + 1) * c->words * 8, hipMemcpyDeviceToHost));
    return FIN_OK;
}

int fin_colors_upload_sets(fin_colors* c, const uint32_t* set_of, const uint64_t* sets, uint64_t n_sets, char* err, size_t errlen) {
    if (!c || !sets || (c->n_unitigs && !set_of)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (n_sets > 0xFFFFFFFEull) { set_err(err, errlen, "at most 2^32 - 2 sets"); return FIN_ELIMIT; }
    const uint32_t W = c->words;
    for (uint32_t w = 0; w < W; w++) if (sets[w]) { set_err(err, errlen, "set 0 is the empty set: its row has a bit set"); return FIN_EINVAL; }
    const uint64_t bad = colors_first_stray(sets, n_sets + 1, c->n_colors, W);
    if (bad != n_sets + 1) { set_err(err, errlen, "set " + std::to_string(bad) + " has a bit at or above n_colors = " + std::to_string(c->n_colors) + " set"); return FIN_EINVAL; }
    for (uint64_t u = 0; u < c->n_unitigs; u++)
        if (set_of[u] > n_sets) { set_err(err, errlen, "unitig " + std::to_string(u) + " has set " + std::to_string(set_of[u]) + ": not in 0 .. n_sets = " + std::to_string(n_sets)); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    if (const int wrc = c->pend.wait(err, errlen)) return wrc;
    void* d_sets = nullptr; void* d_set_of = nullptr;
    if (hipMalloc(&d_sets, (size_t)(n_sets + 1) * W * 8) != hipSuccess || hipMalloc(&d_set_of, (size_t)c->n_unitigs * 4 + 16) != hipSuccess) {
        (void)hipGetLastError(); (void)hipFree(d_sets); set_err(err, errlen, "out of device memory (colour sets)"); return FIN_ENOMEM;
    }
    if (hipMemcpy(d_sets, sets, (size_t)(n_sets + 1) * W * 8, hipMemcpyHostToDevice) != hipSuccess ||
        (c->n_unitigs && hipMemcpy(d_set_of, set_of, (size_t)c->n_unitigs * 4, hipMemcpyHostToDevice) != hipSuccess)) {
        (void)hipFree(d_sets); (void)hipFree(d_set_of); set_err(err, errlen, "copying the colour sets failed"); return FIN_ENODEV;
    }
    (void)hipDeviceSynchronize();           // nothing reads the form that goes any more
    (void)hipFree(c->d_bits); (void)hipFree(c->d_set_of); (void)hipFree(c->d_sets);
    c->d_bits = nullptr; c->d_sets = d_sets; c->d_set_of = d_set_of; c->n_sets = n_sets; c->compact = true;
    for (uint64_t& v : c->cs_stats) v = 0;  // (no table made these sets)
    return FIN_OK;
}

int fin_batch_add_colors(fin_batch* b, fin_colors* c, uint32_t color, void* hip_stream, char* err, size_t errlen) {
    if (!b || !c) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (color >= c->n_colors) { set_err(err, errlen, "colour " + std::to_string(color) + " is not below n_colors = " + std::to_string(c->n_colors)); return FIN_EINVAL; }
    if (const int drc = colors_want_dense(c, err, errlen)) return drc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (const int orc = acc_add_open(b, c, st, err, errlen)) return orc;
    // (no read has a k-mer: the step searched nothing)
    const int rc = b->n_kmers == 0 ? 0 : fin_launch_colors_add(b->last_frec ? b->d_frec : nullptr, (const uint64_t*)b->d_out_offs, b->d_out, (uint32_t)b->n_reads, b->dev.k, c->d_bits,
                                                               c->words, (uint32_t)c->n_unitigs, color, colors_flags(c), b->d_ovf_count, b->last_ovf_cap, st);
    return acc_add_close(c, st, rc, "colour kernel: ", err, errlen);
}

int fin_batch_pseudoalign(fin_batch* b, const fin_colors* c, uint32_t permille, char* err, size_t errlen) {
    if (!b || !c) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int crc = check_permille(permille, BAD_PERMILLE, err, errlen)) return crc;
    if (!b->ran) { set_err(err, errlen, "this batch has not run: there is nothing to pseudoalign (fin_batch_run first)"); return FIN_EINVAL; }
    if (b->idx != c->idx || b->device != c->device) { set_err(err, errlen, "batch and colours belong to different indexes or devices"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    b->psa_ready = false;
    // (no read has a k-mer: the step searched nothing, there is no overflow list to look at -- every row is empty)
    if (b->n_kmers != 0) if (const int orc = batch_overrun_check(b, st, err, errlen)) return orc;   // a run without results: nothing is written
    const uint32_t nr = (uint32_t)b->n_reads;
    if (batch_grow(b, &b->d_psa_rows, b->cap_psa_rows, (size_t)nr * c->words * 8 + 16, st) || batch_grow(b, &b->d_psa_heads, b->cap_psa_heads, (size_t)nr * 16 + 16, st)) {
        set_err(err, errlen, "out of device memory (colour rows of the reads)"); return FIN_ENOMEM;
    }
    if (const int orc = const_cast<fin_colors*>(c)->pend.order(st, err, errlen)) return orc;   // the adds to the matrix, on whichever streams, come first
    const void* const frec = b->n_kmers != 0 && b->last_frec ? b->d_frec : nullptr;
    const int rc = c->compact ? fin_launch_pseudoalign_sets(frec, (const uint64_t*)b->d_out_offs, b->d_out, nr, b->dev.k, c->d_sets, c->words, (uint32_t)c->n_sets,
                                                            (const uint32_t*)c->d_set_of, (uint32_t)c->n_unitigs, permille, b->d_psa_rows, b->d_psa_heads, st)
                              : fin_launch_pseudoalign(frec, (const uint64_t*)b->d_out_offs, b->d_out, nr, b->dev.k, c->d_bits, c->words, (uint32_t)c->n_unitigs, permille,
                                                       b->d_psa_rows, b->d_psa_heads, st);
    if (rc != 0) { set_err(err, errlen, std::string("pseudoalignment kernel: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    b->psa_ready = true; b->psa_words = c->words;
    return FIN_OK;
}

void* fin_batch_device_pseudo_rows(const fin_batch* b) { return b && b->psa_ready ? b->d_psa_rows : nullptr; }
void* fin_batch_device_pseudo_heads(const fin_batch* b) { return b && b->psa_ready ? b->d_psa_heads : nullptr; }

int fin_batch_download_pseudo(fin_batch* b, uint64_t* rows_out, fin_read_pseudo* heads_out, char* err, size_t errlen) {
    if (!b) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (!b->psa_ready) { set_err(err, errlen, "fin_batch_pseudoalign first"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    if (b->n_reads && rows_out) HIPCHK(hipMemcpyAsync(rows_out, b->d_psa_rows, (size_t)b->n_reads * b->psa_words * 8, hipMemcpyDeviceToHost, st));
    if (b->n_reads && heads_out) HIPCHK(hipMemcpyAsync(heads_out, b->d_psa_heads, (size_t)b->n_reads * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FIN_OK;
}

// ---- taxonomic classification: LCA labels, Kraken's rule, tally and clade counts (fin_taxa.hip) -------------------------------------------------
struct fin_taxonomy : fin_acc {
    uint64_t n_unitigs = 0; uint32_t n_taxa = 0;
    uint64_t serial = 0;        // which taxonomy a batch's read taxa were made for
    void* d_parent = nullptr;   // uint32[n_taxa]
    void* d_labels = nullptr;   // uint32[n_unitigs]
    void* d_direct = nullptr;   // the tally: uint64[n_taxa + 1]
    void* d_clade = nullptr;    // uint64[n_taxa], made by every download that asks for it
    std::mutex clade_mu;        // one roll-up at a time goes through d_clade
};
static std::atomic<uint64_t> g_taxonomy_serial{0};

void fin_taxonomy_free(fin_taxonomy* t) {
    if (!acc_free_open(t)) return;
    (void)hipFree(t->d_parent); (void)hipFree(t->d_labels); (void)hipFree(t->d_direct); (void)hipFree(t->d_clade);
    delete t;
}

// the tests of the tree both creates make first, before anything is held against n_taxa
static int taxonomy_check(const uint32_t* parent, uint64_t n_taxa, char* err, size_t errlen) {
    if (n_taxa == 0 || n_taxa > 0x80000000ull) { set_err(err, errlen, "n_taxa is 1 .. 2^31"); return FIN_EINVAL; }
    const uint64_t bad = fin_taxa_first_bad_parent(parent, n_taxa);
    if (bad != n_taxa) {
        set_err(err, errlen, "taxon " + std::to_string(bad) + " has parent " + std::to_string(parent[bad]) +
                                 (bad == 0 ? ": taxon 0 is the root and its own parent" : ": a parent's number is below its child's (topological numbering)"));
        return FIN_EINVAL;
    }
    return FIN_OK;
}
// the buffers the two creates share, behind taxonomy_check: the tree on the device, the tally zeroed, room for the labels.  The caller fills d_labels
static int taxonomy_new(const fin_index* idx, int device, const uint32_t* parent, uint64_t n_taxa, fin_taxonomy** out, char* err, size_t errlen) {
    if (const int orc = acc_create_open(idx, device, nullptr, err, errlen)) return orc;
    fin_taxonomy* t = acc_new<fin_taxonomy>(idx, device, err, errlen);
    if (!t) return FIN_ENOMEM;
    t->n_unitigs = idx->n_unitigs; t->n_taxa = (uint32_t)n_taxa; t->serial = ++g_taxonomy_serial;
    const size_t tally = ((size_t)n_taxa + 1) * 8;
    if (hipMalloc(&t->d_parent, (size_t)n_taxa * 4) != hipSuccess || hipMalloc(&t->d_labels, (size_t)t->n_unitigs * 4 + 16) != hipSuccess ||
        hipMalloc(&t->d_direct, tally) != hipSuccess || hipMalloc(&t->d_clade, (size_t)n_taxa * 8) != hipSuccess) {
        (void)hipGetLastError(); fin_taxonomy_free(t); set_err(err, errlen, "out of device memory (taxonomy, unitig labels and tally)"); return FIN_ENOMEM;
    }
    if (hipMemcpy(t->d_parent, parent, (size_t)n_taxa * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemset(t->d_direct, 0, tally) != hipSuccess) {
        fin_taxonomy_free(t); set_err(err, errlen, "copying the taxonomy failed"); return FIN_ENODEV;
    }
    *out = t;
    return FIN_OK;
}

int fin_taxonomy_create(const fin_index* idx, int device, const uint32_t* parent, uint64_t n_taxa, const uint32_t* unitig_labels, fin_taxonomy** out, char* err,
                        size_t errlen) {
    if (!idx || !out || !parent || (idx->n_unitigs && !unitig_labels)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    *out = nullptr;
    if (const int trc = taxonomy_check(parent, n_taxa, err, errlen)) return trc;
    for (uint64_t u = 0; u < idx->n_unitigs; u++)
        if (unitig_labels[u] != FIN_NO_LABEL && (uint64_t)unitig_labels[u] >= n_taxa) {
            set_err(err, errlen, "unitig " + std::to_string(u) + " has label " + std::to_string(unitig_labels[u]) + ": neither below n_taxa = " + std::to_string(n_taxa) + " nor FIN_NO_LABEL");
            return FIN_EINVAL;
        }
    fin_taxonomy* t = nullptr;
    if (const int rc = taxonomy_new(idx, device, parent, n_taxa, &t, err, errlen)) return rc;
    if (t->n_unitigs && hipMemcpy(t->d_labels, unitig_labels, (size_t)t->n_unitigs * 4, hipMemcpyHostToDevice) != hipSuccess) {
        fin_taxonomy_free(t); set_err(err, errlen, "copying the labels failed"); return FIN_ENODEV;
    }
    *out = t;
    return FIN_OK;
}

int fin_taxonomy_create_from_colors(fin_colors* c, const uint32_t* parent, uint64_t n_taxa, const uint32_t* color_taxon, fin_taxonomy** out, char* err, size_t errlen) {
    if (!c || !out || !parent || !color_taxon) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    *out = nullptr;
    if (const int drc = colors_want_dense(c, err, errlen)) return drc;   // (the labels are made from bits[u * W + w])
    if (const int trc = taxonomy_check(parent, n_taxa, err, errlen)) return trc;
    for (uint32_t q = 0; q < c->n_colors; q++)
        if ((uint64_t)color_taxon[q] >= n_taxa) {
            set_err(err, errlen, "colour " + std::to_string(q) + " has taxon " + std::to_string(color_taxon[q]) + ": not below n_taxa = " + std::to_string(n_taxa));
            return FIN_EINVAL;
        }
    fin_taxonomy* t = nullptr;
    if (const int rc = taxonomy_new(c->idx, c->device, parent, n_taxa, &t, err, errlen)) return rc;
    // the adds to the matrix, on whichever streams, have finished; a withheld step among them is the colours' own refusal
    if (const int orc = acc_download_open(c, colors_flags(c), "a step whose overflow list overran was added: it has no results, nothing of it was coloured (reset the colours)",
                                          nullptr, err, errlen)) { fin_taxonomy_free(t); return orc; }
    void* d_ct = nullptr;
    int rc = FIN_OK;
    if (hipMalloc(&d_ct, (size_t)c->n_colors * 4) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "out of device memory (colour taxa)"); rc = FIN_ENOMEM; }
    else if (hipMemcpy(d_ct, color_taxon, (size_t)c->n_colors * 4, hipMemcpyHostToDevice) != hipSuccess) { set_err(err, errlen, "copying the colour taxa failed"); rc = FIN_ENODEV; }
    else {
        const int lrc = fin_launch_taxa_labels((const uint64_t*)c->d_bits, c->words, (uint32_t)c->n_unitigs, (const uint32_t*)d_ct, (const uint32_t*)t->d_parent,
                                               (uint32_t*)t->d_labels, nullptr);
        const hipError_t e = lrc != 0 ? (hipError_t)lrc : hipStreamSynchronize(nullptr);
        if (e != hipSuccess) { set_err(err, errlen, std::string("unitig LCA kernel: ") + hipGetErrorString(e)); rc = FIN_ENODEV; }
    }
    (void)hipFree(d_ct);
    if (rc != FIN_OK) { fin_taxonomy_free(t); return rc; }
    *out = t;
    return FIN_OK;
}

int fin_taxonomy_reset(fin_taxonomy* t, void* hip_stream) {
    return acc_reset(t, hip_stream, t ? t->d_direct : nullptr, t ? ((size_t)t->n_taxa + 1) * 8 : 0);
}

void* fin_taxonomy_device_labels(const fin_taxonomy* t) { return t ? t->d_labels : nullptr; }

int fin_taxonomy_download_labels(const fin_taxonomy* t, uint32_t* labels_out, char* err, size_t errlen) {
    if (!t || (t->n_unitigs && !labels_out)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(t->device));
    if (t->n_unitigs) HIPCHK(hipMemcpy(labels_out, t->d_labels, (size_t)t->n_unitigs * 4, hipMemcpyDeviceToHost));
    return FIN_OK;
}

int fin_taxonomy_download(fin_taxonomy* t, uint64_t* direct_out, uint64_t* clade_out, uint64_t* total, char* err, size_t errlen) {
    if (!t) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int orc = acc_download_open(t, nullptr, nullptr, nullptr, err, errlen)) return orc;   // (a tally has no flags)
    const size_t n = (size_t)t->n_taxa + 1;
    if (direct_out || total) {
        std::vector<uint64_t> tmp;
        uint64_t* const dst = dst_or_tmp(direct_out, tmp, n);
        HIPCHK(hipMemcpy(dst, t->d_direct, n * 8, hipMemcpyDeviceToHost));
        if (total) *total = sum_of(dst, n, [](uint64_t v) { return v; });
    }
    if (clade_out) {   // the adds have finished: the roll-up runs on the null stream, into the second buffer
        std::lock_guard<std::mutex> g(t->clade_mu);
        HIPCHK(hipMemsetAsync(t->d_clade, 0, (size_t)t->n_taxa * 8, nullptr));
        const int rc = fin_launch_taxa_clades((const uint64_t*)t->d_direct, (const uint32_t*)t->d_parent, t->n_taxa, (uint64_t*)t->d_clade, nullptr);
        if (rc != 0) { set_err(err, errlen, std::string("clade kernel: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
        HIPCHK(hipMemcpy(clade_out, t->d_clade, (size_t)t->n_taxa * 8, hipMemcpyDeviceToHost));
    }
    return FIN_OK;
}

static const char* const BAD_CONFIDENCE = "confidence_permille is a share in thousandths: 0 .. 1000";

int fin_batch_taxa(fin_batch* b, const fin_taxonomy* t, uint32_t min_found, uint32_t confidence_permille, char* err, size_t errlen) {
    if (!b || !t) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int crc = check_permille(confidence_permille, BAD_CONFIDENCE, err, errlen)) return crc;
    if (!b->ran) { set_err(err, errlen, "this batch has not run: there is nothing to classify (fin_batch_run first)"); return FIN_EINVAL; }
    if (b->idx != t->idx || b->device != t->device) { set_err(err, errlen, "batch and taxonomy belong to different indexes or devices"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    b->tax_ready = false;
    // (no read has a k-mer: the step searched nothing, there is no overflow list to look at -- every read is unclassified)
    if (b->n_kmers != 0) if (const int orc = batch_overrun_check(b, st, err, errlen)) return orc;   // a run without results: nothing is written
    const uint32_t nr = (uint32_t)b->n_reads;
    if (batch_grow(b, &b->d_tax, b->cap_tax, (size_t)nr * 16 + 16, st)) { set_err(err, errlen, "out of device memory (read taxa)"); return FIN_ENOMEM; }
    const int rc = fin_launch_taxa_reads(b->n_kmers != 0 && b->last_frec ? b->d_frec : nullptr, (const uint64_t*)b->d_out_offs, b->d_out, nr, b->dev.k,
                                         (const uint32_t*)t->d_labels, (uint32_t)t->n_unitigs, (const uint32_t*)t->d_parent, min_found, confidence_permille, b->d_tax, st);
    if (rc != 0) { set_err(err, errlen, std::string("read taxa kernel: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    b->tax_ready = true; b->tax_serial = t->serial; b->tax_min_found = min_found; b->tax_conf = confidence_permille;
    return FIN_OK;
}

void* fin_batch_device_read_taxa(const fin_batch* b) { return b && b->tax_ready ? b->d_tax : nullptr; }

int fin_batch_download_read_taxa(fin_batch* b, fin_read_taxon* out, char* err, size_t errlen) {
    if (!b || (b->n_reads && !out)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (!b->tax_ready) { set_err(err, errlen, "fin_batch_taxa first"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    if (b->n_reads) HIPCHK(hipMemcpyAsync(out, b->d_tax, (size_t)b->n_reads * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FIN_OK;
}

int fin_batch_add_taxa(fin_batch* b, fin_taxonomy* t, uint32_t min_found, uint32_t confidence_permille, void* hip_stream, char* err, size_t errlen) {
    if (!b || !t) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int crc = check_permille(confidence_permille, BAD_CONFIDENCE, err, errlen)) return crc;
    if (!b->tax_ready || b->tax_serial != t->serial || b->tax_min_found != min_found || b->tax_conf != confidence_permille)
        if (const int rc = fin_batch_taxa(b, t, min_found, confidence_permille, err, errlen)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (const int orc = acc_add_open(b, t, st, err, errlen)) return orc;
    if (const int src = stream_behind(st, b->last_stream, err, errlen)) return src;   // the read taxa were made on the run's stream, behind the run: the add waits for them too
    const int rc = fin_launch_taxa_tally(b->d_tax, (uint32_t)b->n_reads, t->n_taxa, (uint64_t*)t->d_direct, st);
    return acc_add_close(t, st, rc, "taxon tally kernel: ", err, errlen);
}

// ---- paired-end pseudoalignment: one colour row per fragment (fin_paired.hip) -------------------------------------------------------------
static_assert(sizeof(fin_pair_pseudo) == 16, "a fragment's pseudoalignment head is 16 bytes");
int fin_batch_pseudoalign_paired(fin_batch* b, const fin_colors* c, uint32_t permille, uint32_t mode, char* err, size_t errlen) {
    if (!b || !c) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int crc = check_permille(permille, BAD_PERMILLE, err, errlen)) return crc;
    if (const int crc = check_pair_mode(mode, err, errlen)) return crc;
    if (!b->ran) { set_err(err, errlen, "this batch has not run: there is nothing to pseudoalign (fin_batch_run first)"); return FIN_EINVAL; }
    if (b->idx != c->idx || b->device != c->device) { set_err(err, errlen, "batch and colours belong to different indexes or devices"); return FIN_EINVAL; }
    if (const int crc = check_even(b->n_reads, err, errlen)) return crc;
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    b->pair_ready = false;
    if (b->n_kmers != 0) if (const int orc = batch_overrun_check(b, st, err, errlen)) return orc;   // a run without results: nothing is written
    const uint32_t nf = (uint32_t)(b->n_reads / 2);
    if (batch_grow(b, &b->d_pair_rows, b->cap_pair_rows, (size_t)nf * c->words * 8 + 16, st) || batch_grow(b, &b->d_pair_heads, b->cap_pair_heads, (size_t)nf * 16 + 16, st)) {
        set_err(err, errlen, "out of device memory (colour rows of the fragments)"); return FIN_ENOMEM;
    }
    if (const int orc = const_cast<fin_colors*>(c)->pend.order(st, err, errlen)) return orc;   // the adds to the matrix, on whichever streams, come first
    const void* const frec = b->n_kmers != 0 && b->last_frec ? b->d_frec : nullptr;
    const int rc = c->compact ? fin_launch_pseudoalign_paired_sets(frec, (const uint64_t*)b->d_out_offs, b->d_out, nf, b->dev.k, c->d_sets, c->words, (uint32_t)c->n_sets,
                                                                   (const uint32_t*)c->d_set_of, (uint32_t)c->n_unitigs, permille, mode, b->d_pair_rows, b->d_pair_heads, st)
                              : fin_launch_pseudoalign_paired(frec, (const uint64_t*)b->d_out_offs, b->d_out, nf, b->dev.k, c->d_bits, c->words, (uint32_t)c->n_unitigs,
                                                              permille, mode, b->d_pair_rows, b->d_pair_heads, st);
    if (rc != 0) { set_err(err, errlen, std::string("paired pseudoalignment kernel: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    b->pair_ready = true; b->pair_words = c->words;
    return FIN_OK;
}

void* fin_batch_device_pair_rows(const fin_batch* b) { return b && b->pair_ready ? b->d_pair_rows : nullptr; }
void* fin_batch_device_pair_heads(const fin_batch* b) { return b && b->pair_ready ? b->d_pair_heads : nullptr; }

int fin_batch_download_pair_pseudo(fin_batch* b, uint64_t* rows_out, fin_pair_pseudo* heads_out, char* err, size_t errlen) {
    if (!b) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (!b->pair_ready) { set_err(err, errlen, "fin_batch_pseudoalign_paired first"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    const size_t nf = (size_t)(b->n_reads / 2);
    if (nf && rows_out) HIPCHK(hipMemcpyAsync(rows_out, b->d_pair_rows, nf * b->pair_words * 8, hipMemcpyDeviceToHost, st));
    if (nf && heads_out) HIPCHK(hipMemcpyAsync(heads_out, b->d_pair_heads, nf * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FIN_OK;
}

// every device buffer of an estimate (or of a host add's upload), freed on every way out
struct AbBufs {
    std::vector<void*> p;
    ~AbBufs() { for (void* q : p) (void)hipFree(q); }
    void* get(size_t bytes) { void* q = nullptr; if (hipMalloc(&q, bytes ? bytes : 8) != hipSuccess) { (void)hipGetLastError(); return nullptr; } p.push_back(q); return q; }
};
// ---- equivalence classes of pseudoaligned reads (fin_eqclasses.hip) ---------------------------------------------------------------------
struct fin_eqclasses : fin_acc {
    const fin_colors* colors = nullptr;
    uint32_t n_colors = 0, words = 0, lg = 0;
    uint64_t max_classes = 0, slots = 0;
    void* d_tab = nullptr;      // ctr uint64[8] | tags uint64[slots] | counts uint64[slots] | rows uint64[slots * words]
    void* d_scratch = nullptr;  // slot_of uint32[cap_rows] | coll uint32[cap_rows]: kept and only grown
    size_t cap_rows = 0;
    void* d_merge = nullptr;    // fin_eqclasses_merge's scratch, this accumulator being the destination: blk_off | blk_sum | the source's dense rows | reads.  Kept and only grown
    size_t cap_merge = 0;       // (bytes)
    uint32_t tag_bits = 0;      // option "ec_tag_bits" as the first add since the creation or the last reset read it (0: none yet)
    std::mutex mu;              // an add (order, three launches, mark) and a reset are one step each: calls from several host threads take effect in issue order
};
static uint64_t* ec_ctr(const fin_eqclasses* e) { return (uint64_t*)e->d_tab; }
static uint64_t* ec_tags(const fin_eqclasses* e) { return (uint64_t*)e->d_tab + 8; }
static uint64_t* ec_counts(const fin_eqclasses* e) { return ec_tags(e) + e->slots; }
static uint64_t* ec_rows(const fin_eqclasses* e) { return ec_counts(e) + e->slots; }
static size_t ec_zero_bytes(const fin_eqclasses* e) { return (size_t)(8 + 2 * e->slots) * 8; }   // (a slot's row is written when the slot is claimed)

// what a flagged accumulator answers its readers until the reset
static int ec_flagged(const fin_eqclasses* e, const uint64_t* ctr, char* err, size_t errlen) {
    if (ctr[4] & 1u) { set_err(err, errlen, "a row with a bit at or above n_colors was added (not counted; reset the accumulator)"); return FIN_EINVAL; }
    if ((ctr[4] & 2u) || ctr[2] > e->max_classes) { set_err(err, errlen, "more than max_classes distinct rows (max_classes = " + std::to_string(e->max_classes) + "; reset the accumulator)"); return FIN_ELIMIT; }
    return FIN_OK;
}

void fin_eqclasses_free(fin_eqclasses* e) {
    if (!acc_free_open(e)) return;
    (void)hipFree(e->d_tab); (void)hipFree(e->d_scratch); (void)hipFree(e->d_merge);
    delete e;
}

int fin_eqclasses_create(const fin_colors* c, uint64_t max_classes, fin_eqclasses** out, char* err, size_t errlen) {
    if (!c || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    *out = nullptr;
    if (max_classes == 0 || max_classes > (1ull << 26)) { set_err(err, errlen, "max_classes is 1 .. 2^26"); return FIN_ELIMIT; }
    HIPCHK(hipSetDevice(c->device));   // (not acc_create_open: it goes beside a colour matrix, which has passed those checks)
    fin_eqclasses* e = acc_new<fin_eqclasses>(c->idx, c->device, err, errlen);
    if (!e) return FIN_ENOMEM;
    e->colors = c; e->n_colors = c->n_colors; e->words = c->words; e->max_classes = max_classes;
    e->lg = 1;
    while ((1ull << e->lg) < 2 * max_classes) e->lg++;
    e->slots = 1ull << e->lg;
    const size_t bytes = ec_zero_bytes(e) + (size_t)e->slots * e->words * 8;
    if (const int arc = acc_alloc_zero(e, &e->d_tab, bytes, ec_zero_bytes(e), "out of device memory (table of equivalence classes)", fin_eqclasses_free, err, errlen)) return arc;
    *out = e;
    return FIN_OK;
}

int fin_eqclasses_reset(fin_eqclasses* e, void* hip_stream) {
    if (!e) return FIN_EINVAL;
    if (hipSetDevice(e->device) != hipSuccess) return FIN_ENODEV;
    std::lock_guard<std::mutex> g(e->mu);
    e->tag_bits = 0;
    return acc_reset(e, hip_stream, e->d_tab, ec_zero_bytes(e));
}

// the add proper, on `st`: behind every add and reset issued so far, whichever streams they were given.  With the accumulator's lock held.  d_weights null: every
// row counts once (fin_launch_ec_add); else row r counts d_weights[r] times and n_unaligned all-zero rows are counted besides (fin_launch_ec_add_classes)
static int ec_add_locked(fin_eqclasses* e, const void* d_rows, const void* d_weights, uint64_t n_rows, uint64_t n_unaligned, hipStream_t st, char* err, size_t errlen) {
    if (n_rows > e->cap_rows) {   // (the adds under way use the old scratch)
        if (const int wrc = e->pend.wait(err, errlen)) return wrc;
        (void)hipFree(e->d_scratch); e->d_scratch = nullptr; e->cap_rows = 0;
        const size_t want = (size_t)n_rows + (size_t)n_rows / 8 + 64;
        if (hipMalloc(&e->d_scratch, want * 8) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "out of device memory (scratch of the equivalence classes)"); return FIN_ENOMEM; }
        e->cap_rows = want;
    }
    if (e->tag_bits == 0) e->tag_bits = (uint32_t)optv(e->idx, O_ec_tag_bits);
    if (const int orc = e->pend.order(st, err, errlen)) return orc;
    int rc = 0;
    if (d_weights || n_unaligned)
        rc = fin_launch_ec_add_classes(d_rows, d_weights, (uint32_t)n_rows, n_unaligned, e->words, e->n_colors, ec_tags(e), ec_counts(e), ec_rows(e), e->lg, e->max_classes,
                                       e->tag_bits, ec_ctr(e), (uint32_t*)e->d_scratch, (uint32_t*)e->d_scratch + e->cap_rows, st);
    else if (n_rows)
        rc = fin_launch_ec_add(d_rows, (uint32_t)n_rows, e->words, e->n_colors, ec_tags(e), ec_counts(e), ec_rows(e), e->lg, e->max_classes, e->tag_bits,
                               (uint32_t)optv(e->idx, O_ec_combine), ec_ctr(e), (uint32_t*)e->d_scratch, (uint32_t*)e->d_scratch + e->cap_rows, st);
    if (rc != 0) { set_err(err, errlen, std::string("equivalence class kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    return e->pend.mark(st, err, errlen);
}
static int ec_add_rows(fin_eqclasses* e, const void* d_rows, uint64_t n_rows, hipStream_t st, char* err, size_t errlen, const void* d_weights = nullptr,
                       uint64_t n_unaligned = 0) {
    if (n_rows >= 0x80000000ull) { set_err(err, errlen, "more than 2^31-1 rows in one add"); return FIN_ELIMIT; }
    std::lock_guard<std::mutex> g(e->mu);
    return ec_add_locked(e, d_rows, d_weights, n_rows, n_unaligned, st, err, errlen);
}

int fin_eqclasses_add_rows(fin_eqclasses* e, const void* d_rows, uint64_t n_rows, void* hip_stream, char* err, size_t errlen) {
    if (!e || (n_rows && !d_rows)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    return ec_add_rows(e, d_rows, n_rows, (hipStream_t)hip_stream, err, errlen);
}

int fin_eqclasses_add_classes(fin_eqclasses* e, const void* d_rows, const void* d_reads, uint64_t n_classes, uint64_t n_unaligned, void* hip_stream, char* err,
                              size_t errlen) {
    if (!e || (n_classes && (!d_rows || !d_reads))) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    return ec_add_rows(e, d_rows, n_classes, (hipStream_t)hip_stream, err, errlen, n_classes ? d_reads : nullptr, n_unaligned);
}

// the first row of n with a bit at or above n_colors; n: none
static uint64_t ec_first_stray(const uint64_t* rows, uint64_t n, uint32_t n_colors, uint32_t W) {
    const uint64_t stray = (n_colors & 63u) ? ~0ull << (n_colors & 63u) : 0ull;
    for (uint64_t r = 0; r < n; r++) if (rows[r * W + (W - 1)] & stray) return r;
    return n;
}

int fin_eqclasses_add_classes_host(fin_eqclasses* e, const uint64_t* rows, const uint64_t* reads, uint64_t n_classes, uint64_t n_unaligned, char* err, size_t errlen) {
    if (!e || (n_classes && (!rows || !reads))) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (n_classes >= 0x80000000ull) { set_err(err, errlen, "more than 2^31-1 classes in one add"); return FIN_ELIMIT; }
    const uint64_t bad = ec_first_stray(rows, n_classes, e->n_colors, e->words);
    if (bad != n_classes) { set_err(err, errlen, "class " + std::to_string(bad) + " has a bit at or above n_colors = " + std::to_string(e->n_colors) + " set (nothing was added)"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    AbBufs bufs;   // (freed on every way out)
    uint64_t* d = nullptr;
    if (n_classes) {
        const size_t n = (size_t)n_classes, W = e->words;
        d = (uint64_t*)bufs.get(n * (W + 1) * 8);
        if (!d) { set_err(err, errlen, "out of device memory (classes to add)"); return FIN_ENOMEM; }
        HIPCHK(hipMemcpy(d, rows, n * W * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d + n * W, reads, n * 8, hipMemcpyHostToDevice));
    }
    if (const int rc = ec_add_rows(e, d, n_classes, nullptr, err, errlen, d ? d + (size_t)n_classes * e->words : nullptr, n_unaligned)) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));   // the device copy is freed behind the add; the caller's arrays were free since the copies
    return FIN_OK;
}

int fin_eqclasses_merge(fin_eqclasses* dst, fin_eqclasses* src, void* hip_stream, char* err, size_t errlen) {
    if (!dst || !src) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (dst == src) { set_err(err, errlen, "an accumulator cannot be merged into itself"); return FIN_EINVAL; }
    if (dst->device != src->device) { set_err(err, errlen, "the accumulators are on different devices (fin_eqclasses_download and fin_eqclasses_add_classes_host carry classes between devices)"); return FIN_EINVAL; }
    if (dst->n_colors != src->n_colors) { set_err(err, errlen, "the accumulators have different n_colors (" + std::to_string(dst->n_colors) + " and " + std::to_string(src->n_colors) + ")"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(dst->device));
    hipStream_t st = (hipStream_t)hip_stream;
    // both locks, in a fixed order: two merges in opposite directions from two host threads do not wait for each other
    fin_eqclasses* const first = std::less<fin_eqclasses*>()(dst, src) ? dst : src;
    fin_eqclasses* const second = first == dst ? src : dst;
    std::lock_guard<std::mutex> g1(first->mu);
    std::lock_guard<std::mutex> g2(second->mu);
    if (const int wrc = src->pend.wait(err, errlen)) return wrc;
    uint64_t ctr[8];
    HIPCHK(hipMemcpy(ctr, ec_ctr(src), sizeof ctr, hipMemcpyDeviceToHost));
    if (const int frc = ec_flagged(src, ctr, err, errlen)) return frc;
    // the source's occupied slots are its classes, ctr[2]: a slot's tag is written exactly where the class counter is bumped (claim pass, serial pass) and both
    // are zeroed together.  So the dense list's length is known without a look at the scan's total, and nothing here waits for the destination
    const uint64_t n = ctr[2];
    const uint32_t W = src->words, nb = fin_ec_blocks((uint32_t)src->slots);
    const size_t off_bytes = (size_t)nb * 8 + 8, sum_bytes = ((size_t)nb * 4 + 7) & ~(size_t)7, want = off_bytes + sum_bytes + (size_t)n * (W + 1) * 8;
    if (n && want > dst->cap_merge) {   // (an earlier merge's add may still read the old list)
        if (const int wrc = dst->pend.wait(err, errlen)) return wrc;
        (void)hipFree(dst->d_merge); dst->d_merge = nullptr; dst->cap_merge = 0;
        if (hipMalloc(&dst->d_merge, want + want / 8) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "out of device memory (the dense class list of a merge)"); return FIN_ENOMEM; }
        dst->cap_merge = want + want / 8;
    }
    uint64_t* d_rows = nullptr;
    if (n) {
        uint64_t* const d_off = (uint64_t*)dst->d_merge; uint64_t* const d_total = d_off + nb; uint32_t* const d_sum = (uint32_t*)((char*)dst->d_merge + off_bytes);
        d_rows = (uint64_t*)((char*)dst->d_merge + off_bytes + sum_bytes);
        if (const int orc = dst->pend.order(st, err, errlen)) return orc;   // the scratch is free once the destination's earlier adds have run
        int rc = fin_launch_ec_occupied(ec_tags(src), (uint32_t)src->slots, d_sum, d_off, d_total, st);
        if (rc == 0) rc = fin_launch_ec_gather(ec_tags(src), ec_counts(src), ec_rows(src), (uint32_t)src->slots, W, d_off, d_rows, d_rows + (size_t)n * W, st);
        if (rc != 0) { set_err(err, errlen, std::string("compaction of the equivalence classes: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
        if (const int mrc = src->pend.mark(st, err, errlen)) return mrc;   // a later add or reset of the source runs behind the gather
    }
    return ec_add_locked(dst, d_rows, n ? d_rows + (size_t)n * W : nullptr, n, ctr[1], st, err, errlen);
}

int fin_batch_add_eqclasses(fin_batch* b, fin_eqclasses* e, uint32_t permille, void* hip_stream, char* err, size_t errlen) {
    if (!b || !e) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    // always: the batch does not remember which matrix and threshold its rows belong to, and the matrix may have changed
    if (const int rc = fin_batch_pseudoalign(b, e->colors, permille, err, errlen)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (const int src = stream_behind(st, b->last_stream, err, errlen)) return src;   // the rows were made on the run's stream, behind the run: the add waits for them
    return ec_add_rows(e, b->d_psa_rows, b->n_reads, st, err, errlen);
}

int fin_batch_add_eqclasses_paired(fin_batch* b, fin_eqclasses* e, uint32_t permille, uint32_t mode, void* hip_stream, char* err, size_t errlen) {
    if (!b || !e) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    // always, as fin_batch_add_eqclasses does: the batch does not remember which matrix, threshold and mode its rows belong to
    if (const int rc = fin_batch_pseudoalign_paired(b, e->colors, permille, mode, err, errlen)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (const int src = stream_behind(st, b->last_stream, err, errlen)) return src;   // the rows were made on the run's stream, behind the run: the add waits for them
    return ec_add_rows(e, b->d_pair_rows, b->n_reads / 2, st, err, errlen);   // a fragment is one row
}

int fin_eqclasses_stats(fin_eqclasses* e, uint64_t out[4], char* err, size_t errlen) {
    if (!e || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    if (const int wrc = e->pend.wait(err, errlen)) return wrc;
    HIPCHK(hipMemcpy(out, ec_ctr(e), 32, hipMemcpyDeviceToHost));
    return FIN_OK;
}

// canonical order: ascending by word 0, then word 1 ..., unsigned -- np.unique(rows, axis=0)'s.  perm[i] = the i-th class's place in rows
static void ec_canonical(const uint64_t* rows, uint64_t n, uint32_t W, std::vector<uint64_t>& perm) {
    perm.resize((size_t)n);
    for (uint64_t i = 0; i < n; i++) perm[(size_t)i] = i;
    std::sort(perm.begin(), perm.end(), [&](uint64_t a, uint64_t b) { return std::lexicographical_compare(rows + a * W, rows + a * W + W, rows + b * W, rows + b * W + W); });
}

int fin_eqclasses_download(fin_eqclasses* e, uint64_t* rows_out, uint64_t* reads_out, uint64_t cap, uint64_t* n_classes, uint64_t* n_unaligned, char* err, size_t errlen) {
    if (!e || !n_classes || (cap && (!rows_out || !reads_out))) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    if (const int wrc = e->pend.wait(err, errlen)) return wrc;
    uint64_t ctr[8];
    HIPCHK(hipMemcpy(ctr, ec_ctr(e), sizeof ctr, hipMemcpyDeviceToHost));
    if (const int frc = ec_flagged(e, ctr, err, errlen)) return frc;
    // compaction on the device: the occupied slots counted per block, scanned, gathered into a dense list -- the table itself never crosses PCIe
    const uint32_t W = e->words, nb = fin_ec_blocks((uint32_t)e->slots);
    void* d_tmp = nullptr; void* d_dense = nullptr;
    const size_t off_bytes = (size_t)nb * 8 + 8, sum_bytes = (size_t)nb * 4;
    if (hipMalloc(&d_tmp, off_bytes + sum_bytes) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "out of device memory (compaction of the equivalence classes)"); return FIN_ENOMEM; }
    uint64_t* const d_off = (uint64_t*)d_tmp; uint64_t* const d_total = d_off + nb; uint32_t* const d_sum = (uint32_t*)((char*)d_tmp + off_bytes);
    int rc = fin_launch_ec_occupied(ec_tags(e), (uint32_t)e->slots, d_sum, d_off, d_total, nullptr);
    uint64_t total = 0;
    hipError_t he = rc == 0 ? hipMemcpy(&total, d_total, 8, hipMemcpyDeviceToHost) : (hipError_t)rc;
    std::vector<uint64_t> rows, reads;
    if (he == hipSuccess && total) {
        rows.resize((size_t)total * W); reads.resize((size_t)total);
        he = hipMalloc(&d_dense, (size_t)total * (W + 1) * 8);
        if (he == hipSuccess) {
            rc = fin_launch_ec_gather(ec_tags(e), ec_counts(e), ec_rows(e), (uint32_t)e->slots, W, d_off, d_dense, (uint64_t*)d_dense + total * W, nullptr);
            he = rc == 0 ? hipMemcpy(rows.data(), d_dense, (size_t)total * W * 8, hipMemcpyDeviceToHost) : (hipError_t)rc;
            if (he == hipSuccess) he = hipMemcpy(reads.data(), (uint64_t*)d_dense + total * W, (size_t)total * 8, hipMemcpyDeviceToHost);
        }
    }
    (void)hipFree(d_tmp); (void)hipFree(d_dense);
    if (he != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, std::string("compaction of the equivalence classes: ") + hipGetErrorString(he)); return FIN_ENODEV; }
    *n_classes = total;
    if (n_unaligned) *n_unaligned = ctr[1];
    if (total > cap) { set_err(err, errlen, "room for " + std::to_string(cap) + " classes, " + std::to_string(total) + " needed"); return FIN_ELIMIT; }
    std::vector<uint64_t> perm;
    ec_canonical(rows.data(), total, W, perm);
    for (uint64_t i = 0; i < total; i++) {
        memcpy(rows_out + i * W, rows.data() + perm[(size_t)i] * W, (size_t)W * 8);
        reads_out[i] = reads[(size_t)perm[(size_t)i]];
    }
    return FIN_OK;
}

// host: the CPU statement of the accumulator -- the rows sorted, runs of equal rows counted
int fin_rows_eqclasses(const uint64_t* rows, uint64_t n_rows, uint32_t n_colors, uint64_t* rows_out, uint64_t* reads_out, uint64_t cap, uint64_t* n_classes,
                       uint64_t* n_unaligned) {
    if (n_colors == 0 || n_colors > FIN_MAX_COLORS) return FIN_ELIMIT;
    if ((n_rows && !rows) || !n_classes || (cap && (!rows_out || !reads_out))) return FIN_EINVAL;
    const uint32_t W = (n_colors + 63u) / 64u;
    const uint64_t stray = (n_colors & 63u) ? ~0ull << (n_colors & 63u) : 0ull;
    std::vector<uint64_t> live;
    uint64_t n_un = 0;
    for (uint64_t r = 0; r < n_rows; r++) {
        const uint64_t* row = rows + r * W;
        if (row[W - 1] & stray) return FIN_EINVAL;
        bool ne = false;
        for (uint32_t w = 0; w < W; w++) if (row[w]) ne = true;
        if (ne) live.push_back(r); else n_un++;
    }
    std::sort(live.begin(), live.end(), [&](uint64_t a, uint64_t b) { return std::lexicographical_compare(rows + a * W, rows + a * W + W, rows + b * W, rows + b * W + W); });
    uint64_t n = 0;
    for (size_t i = 0; i < live.size();) {
        size_t j = i + 1;
        while (j < live.size() && !memcmp(rows + live[i] * W, rows + live[j] * W, (size_t)W * 8)) j++;
        if (n < cap) { memcpy(rows_out + n * W, rows + live[i] * W, (size_t)W * 8); reads_out[n] = (uint64_t)(j - i); }
        n++; i = j;
    }
    *n_classes = n;
    if (n_unaligned) *n_unaligned = n_un;
    return n > cap ? FIN_ELIMIT : FIN_OK;
}

// host twin of the weighted add and of fin_eqclasses_merge: the classes of the union of two class lists -- both lists' non-empty rows with reads > 0 sorted, the
// reads of runs of equal rows summed
int fin_classes_merge(const uint64_t* rows_a, const uint64_t* reads_a, uint64_t n_a, const uint64_t* rows_b, const uint64_t* reads_b, uint64_t n_b, uint32_t n_colors,
                      uint64_t* rows_out, uint64_t* reads_out, uint64_t cap, uint64_t* n_classes) {
    if (n_colors == 0 || n_colors > FIN_MAX_COLORS) return FIN_ELIMIT;
    if ((n_a && (!rows_a || !reads_a)) || (n_b && (!rows_b || !reads_b)) || !n_classes || (cap && (!rows_out || !reads_out))) return FIN_EINVAL;
    const uint32_t W = (n_colors + 63u) / 64u;
    if (ec_first_stray(rows_a, n_a, n_colors, W) != n_a || ec_first_stray(rows_b, n_b, n_colors, W) != n_b) return FIN_EINVAL;
    std::vector<std::pair<const uint64_t*, uint64_t>> live;   // {row, reads}
    const auto take = [&](const uint64_t* rows, const uint64_t* reads, uint64_t n) {
        for (uint64_t r = 0; r < n; r++) {
            const uint64_t* row = rows + r * W;
            bool ne = false;
            for (uint32_t w = 0; w < W; w++) if (row[w]) ne = true;
            if (ne && reads[r]) live.push_back({row, reads[r]});
        }
    };
    take(rows_a, reads_a, n_a); take(rows_b, reads_b, n_b);
    std::sort(live.begin(), live.end(), [&](const std::pair<const uint64_t*, uint64_t>& a, const std::pair<const uint64_t*, uint64_t>& b) {
        return std::lexicographical_compare(a.first, a.first + W, b.first, b.first + W);
    });
    uint64_t n = 0;
    for (size_t i = 0; i < live.size();) {
        size_t j = i;
        uint64_t sum = 0;
        while (j < live.size() && !memcmp(live[i].first, live[j].first, (size_t)W * 8)) sum += live[j++].second;
        if (n < cap) { memcpy(rows_out + n * W, live[i].first, (size_t)W * 8); reads_out[n] = sum; }
        n++; i = j;
    }
    *n_classes = n;
    return n > cap ? FIN_ELIMIT : FIN_OK;
}

// host: reads_with[c] = the reads of the classes that contain colour c; reads_only[c] = the reads of the class {c}
int fin_eqclasses_color_tally(const uint64_t* class_rows, const uint64_t* class_reads, uint64_t n_classes, uint32_t n_colors, uint64_t* reads_with, uint64_t* reads_only) {
    if (n_colors == 0 || n_colors > FIN_MAX_COLORS) return FIN_ELIMIT;
    if ((n_classes && (!class_rows || !class_reads)) || !reads_with || !reads_only) return FIN_EINVAL;
    const uint32_t W = (n_colors + 63u) / 64u;
    const uint64_t stray = (n_colors & 63u) ? ~0ull << (n_colors & 63u) : 0ull;
    for (uint64_t i = 0; i < n_classes; i++) if (class_rows[i * W + (W - 1)] & stray) return FIN_EINVAL;
    for (uint32_t c = 0; c < n_colors; c++) reads_with[c] = reads_only[c] = 0;
    for (uint64_t i = 0; i < n_classes; i++) {
        const uint64_t* row = class_rows + i * W;
        uint32_t pc = 0, last = 0;
        for (uint32_t w = 0; w < W; w++)
            for (uint64_t m = row[w]; m; m &= m - 1) { last = 64u * w + (uint32_t)__builtin_ctzll(m); reads_with[last] += class_reads[i]; pc++; }
        if (pc == 1u) reads_only[last] += class_reads[i];
    }
    return FIN_OK;
}

// ---- reads assigned to references from per-colour weights (fin_assign.hip) ------------------------------------------------
static_assert(sizeof(fin_read_assign) == 8, "an assignment head is 8 bytes");
struct fin_assign : fin_acc {
    const fin_colors* colors = nullptr;
    uint32_t n_colors = 0, words = 0;
    void* d_cnt = nullptr;      // assigned uint64[n_colors] | sole uint64[n_colors] | counters uint64[4]: what a reset zeroes
    void* d_w = nullptr;        // x double[64 words] | thr double[64 words], 0 behind n_colors
    std::mutex mu;              // a set and an add are one step each
};
static size_t asg_cnt_bytes(const fin_assign* a) { return ((size_t)2 * a->n_colors + 4) * 8; }
static uint64_t* asg_assigned(const fin_assign* a) { return (uint64_t*)a->d_cnt; }
static uint64_t* asg_sole(const fin_assign* a) { return (uint64_t*)a->d_cnt + a->n_colors; }
static uint64_t* asg_counters(const fin_assign* a) { return (uint64_t*)a->d_cnt + 2 * (size_t)a->n_colors; }
static double* asg_x(const fin_assign* a) { return (double*)a->d_w; }
static double* asg_thr(const fin_assign* a) { return (double*)a->d_w + 64u * (size_t)a->words; }

static int asg_check(uint32_t n_colors, const double* weights, const double* thresholds, char* err, size_t errlen) {
    int what = 0;
    const uint32_t bad = fin_assign_first_bad(weights, thresholds, n_colors, &what);
    if (bad == n_colors) return FIN_OK;
    set_err(err, errlen, what == 0 ? "the weight of colour " + std::to_string(bad) + " is not a finite number >= 0"
                                   : "the threshold of colour " + std::to_string(bad) + " is not a number in 0 .. 1");
    return FIN_EINVAL;
}
// the new weights and thresholds, on `st` behind every add issued so far; returns when they are in place, so every later add finds them
static int asg_upload(fin_assign* a, const double* weights, const double* thresholds, hipStream_t st, char* err, size_t errlen) {
    const size_t pad = 64u * (size_t)a->words;
    std::vector<double> h(2 * pad, 0.0);
    for (uint32_t c = 0; c < a->n_colors; c++) { h[c] = weights[c]; h[pad + c] = thresholds[c]; }
    if (const int orc = a->pend.order(st, err, errlen)) return orc;
    HIPCHK(hipMemcpyAsync(a->d_w, h.data(), h.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return FIN_OK;
}

void fin_assign_free(fin_assign* a) {
    if (!acc_free_open(a)) return;
    (void)hipFree(a->d_cnt); (void)hipFree(a->d_w);
    delete a;
}

int fin_assign_create(const fin_colors* c, const double* weights, const double* thresholds, fin_assign** out, char* err, size_t errlen) {
    if (!c || !weights || !thresholds || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    *out = nullptr;
    if (const int crc = asg_check(c->n_colors, weights, thresholds, err, errlen)) return crc;
    HIPCHK(hipSetDevice(c->device));   // (not acc_create_open: it goes beside a colour matrix, which has passed those checks)
    fin_assign* a = acc_new<fin_assign>(c->idx, c->device, err, errlen);
    if (!a) return FIN_ENOMEM;
    a->colors = c; a->n_colors = c->n_colors; a->words = c->words;
    if (const int arc = acc_alloc_zero(a, &a->d_cnt, asg_cnt_bytes(a), asg_cnt_bytes(a), "out of device memory (assignment counts)", fin_assign_free, err, errlen)) return arc;
    if (hipMalloc(&a->d_w, (size_t)a->words * 1024u) != hipSuccess) { (void)hipGetLastError(); fin_assign_free(a); set_err(err, errlen, "out of device memory (assignment weights)"); return FIN_ENOMEM; }
    if (const int urc = asg_upload(a, weights, thresholds, nullptr, err, errlen)) { fin_assign_free(a); return urc; }
    *out = a;
    return FIN_OK;
}

int fin_assign_reset(fin_assign* a, void* hip_stream) {
    return acc_reset(a, hip_stream, a ? a->d_cnt : nullptr, a ? asg_cnt_bytes(a) : 0);
}

int fin_assign_set(fin_assign* a, const double* weights, const double* thresholds, void* hip_stream, char* err, size_t errlen) {
    if (!a || !weights || !thresholds) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int crc = asg_check(a->n_colors, weights, thresholds, err, errlen)) return crc;
    HIPCHK(hipSetDevice(a->device));
    std::lock_guard<std::mutex> g(a->mu);
    return asg_upload(a, weights, thresholds, (hipStream_t)hip_stream, err, errlen);
}

// the add proper, on `st`: behind the accumulator's last reset (a set has finished when it returns)
static int asg_add_rows(fin_assign* a, const void* d_rows, uint64_t n_rows, void* d_out_rows, void* d_heads, hipStream_t st, char* err, size_t errlen) {
    if (n_rows > 0xFFFFFFFFull) { set_err(err, errlen, "more than 2^32-1 rows in one add"); return FIN_ELIMIT; }
    std::lock_guard<std::mutex> g(a->mu);
    if (const int brc = a->pend.behind_reset(st, err, errlen)) return brc;
    const int rc = fin_launch_assign_rows(d_rows, n_rows, a->words, a->n_colors, (uint32_t)optv(a->idx, O_assign_rpb), asg_x(a), asg_thr(a), d_out_rows, d_heads,
                                          asg_assigned(a), asg_sole(a), asg_counters(a), st);
    return acc_add_close(a, st, rc, "assignment kernel: ", err, errlen);
}

int fin_assign_rows(fin_assign* a, const void* rows_dev, uint64_t n_rows, void* out_rows_dev, void* heads_dev, void* hip_stream, char* err, size_t errlen) {
    if (!a || (n_rows && !rows_dev)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(a->device));
    return asg_add_rows(a, rows_dev, n_rows, out_rows_dev, heads_dev, (hipStream_t)hip_stream, err, errlen);
}

int fin_assign_download(fin_assign* a, uint64_t* assigned, uint64_t* sole, uint64_t counters[4], char* err, size_t errlen) {
    if (!a) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int orc = acc_download_open(a, nullptr, nullptr, nullptr, err, errlen)) return orc;   // (the counts have no flags)
    if (assigned) HIPCHK(hipMemcpy(assigned, asg_assigned(a), (size_t)a->n_colors * 8, hipMemcpyDeviceToHost));
    if (sole) HIPCHK(hipMemcpy(sole, asg_sole(a), (size_t)a->n_colors * 8, hipMemcpyDeviceToHost));
    if (counters) HIPCHK(hipMemcpy(counters, asg_counters(a), 32, hipMemcpyDeviceToHost));
    return FIN_OK;
}

static int check_assign_unit(uint32_t unit, char* err, size_t errlen) {
    if (unit > 2u) { set_err(err, errlen, "unit is 0 (reads), 1 (pairs, FIN_PAIR_ANY) or 2 (pairs, FIN_PAIR_BOTH)"); return FIN_EINVAL; }
    return FIN_OK;
}

int fin_batch_assign(fin_batch* b, fin_assign* a, uint32_t permille, uint32_t unit, void* hip_stream, char* err, size_t errlen) {
    if (!b || !a) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int crc = check_assign_unit(unit, err, errlen)) return crc;
    // always, as fin_batch_add_eqclasses does: the batch does not remember which matrix, threshold and mode its rows belong to
    if (const int rc = unit == 0u ? fin_batch_pseudoalign(b, a->colors, permille, err, errlen)
                                  : fin_batch_pseudoalign_paired(b, a->colors, permille, unit == 1u ? FIN_PAIR_ANY : FIN_PAIR_BOTH, err, errlen)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    b->asg_ready = false; b->bin_ready = false;
    const uint64_t n = unit == 0u ? b->n_reads : b->n_reads / 2;
    const void* const d_rows = unit == 0u ? b->d_psa_rows : b->d_pair_rows;
    // (an earlier assignment's readers ran on its stream: a buffer that grows is freed behind them)
    if (batch_grow(b, &b->d_asg_rows, b->cap_asg_rows, (size_t)n * a->words * 8 + 16, b->asg_stream) || batch_grow(b, &b->d_asg_heads, b->cap_asg_heads, (size_t)n * 8 + 16, b->asg_stream)) {
        set_err(err, errlen, "out of device memory (assigned rows)"); return FIN_ENOMEM;
    }
    if (const int src = stream_behind(st, b->last_stream, err, errlen)) return src;   // the rows were made on the run's stream, behind the run: the add waits for them
    if (b->asg_stream != st) if (const int src = stream_behind(st, b->asg_stream, err, errlen)) return src;   // ... and the buffers' earlier readers come first
    if (const int rc = asg_add_rows(a, d_rows, n, b->d_asg_rows, b->d_asg_heads, st, err, errlen)) return rc;
    b->asg_ready = true; b->asg_words = a->words; b->asg_colors = a->n_colors; b->asg_n = n; b->asg_stream = st;
    return FIN_OK;
}

void* fin_batch_device_assign_rows(const fin_batch* b) { return b && b->asg_ready ? b->d_asg_rows : nullptr; }
void* fin_batch_device_assign_heads(const fin_batch* b) { return b && b->asg_ready ? b->d_asg_heads : nullptr; }

int fin_batch_download_assign(fin_batch* b, uint64_t* rows_out, fin_read_assign* heads_out, char* err, size_t errlen) {
    if (!b) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (!b->asg_ready) { set_err(err, errlen, "fin_batch_assign first"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->asg_stream;
    if (b->asg_n && rows_out) HIPCHK(hipMemcpyAsync(rows_out, b->d_asg_rows, (size_t)b->asg_n * b->asg_words * 8, hipMemcpyDeviceToHost, st));
    if (b->asg_n && heads_out) HIPCHK(hipMemcpyAsync(heads_out, b->d_asg_heads, (size_t)b->asg_n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FIN_OK;
}

int fin_batch_assign_bin(fin_batch* b, uint32_t colour, uint64_t* n_ids, char* err, size_t errlen) {
    if (!b) { set_err(err, errlen, "null batch"); return FIN_EINVAL; }
    if (!b->asg_ready) { set_err(err, errlen, "fin_batch_assign first"); return FIN_EINVAL; }
    if (colour >= b->asg_colors) { set_err(err, errlen, "colour " + std::to_string(colour) + " is not below n_colors = " + std::to_string(b->asg_colors)); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->asg_stream;
    b->bin_ready = false;
    const uint32_t n = (uint32_t)b->asg_n, nb = fin_rsm_blocks(n);
    if (batch_grow(b, &b->d_bin_bits, b->cap_bin_bits, (size_t)((n + 63u) / 64u) * 8 + 8, st) || batch_grow(b, &b->d_bin_bsum, b->cap_bin_bsum, (size_t)nb * 4 + 4, st) ||
        batch_grow(b, &b->d_bin_boff, b->cap_bin_boff, (size_t)nb * 8 + 8, st)) {
        set_err(err, errlen, "out of device memory (bin tables)"); return FIN_ENOMEM;
    }
    uint64_t* const d_total = (uint64_t*)b->d_bin_boff + nb;   // (behind the block offsets)
    int rc = fin_launch_assign_column(b->d_asg_rows, n, b->asg_words, colour, (uint64_t*)b->d_bin_bits, (uint32_t*)b->d_bin_bsum, (uint64_t*)b->d_bin_boff, d_total, st);
    if (rc != 0) { set_err(err, errlen, std::string("bin kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (total > n) { set_err(err, errlen, "bin kernels: more rows in the bin than rows"); return FIN_ENODEV; }
    if (batch_grow(b, &b->d_bin_ids, b->cap_bin_ids, (size_t)total * 4 + 16, st)) { set_err(err, errlen, "out of device memory (bin ids)"); return FIN_ENOMEM; }
    rc = fin_launch_screen_ids((const uint64_t*)b->d_bin_bits, (const uint64_t*)b->d_bin_boff, n, (uint32_t*)b->d_bin_ids, st);
    if (rc != 0) { set_err(err, errlen, std::string("bin kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    b->n_bin = total; b->bin_ready = true;
    if (n_ids) *n_ids = total;
    return FIN_OK;
}

void* fin_batch_device_bin_ids(const fin_batch* b) { return b && b->bin_ready ? b->d_bin_ids : nullptr; }

int fin_batch_download_bin(fin_batch* b, uint32_t* ids_out, char* err, size_t errlen) {
    if (!b || (b->bin_ready && b->n_bin && !ids_out)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (!b->bin_ready) { set_err(err, errlen, "fin_batch_assign_bin first"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->asg_stream;
    if (b->n_bin) HIPCHK(hipMemcpyAsync(ids_out, b->d_bin_ids, (size_t)b->n_bin * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FIN_OK;
}

// ---- abundances from the classes (fin_abundance.hip) ---------------------------------------------------------------------
#define FIN_AB_MAX_ITERS 100000u
#define FIN_AB_GROUP 32u   // iterations enqueued between two looks at the device's {done, iters}
static int ab_check_args(uint32_t n_colors, const double* lengths, uint32_t max_iters, double tol, char* err, size_t errlen) {
    if (n_colors == 0 || n_colors > FIN_MAX_COLORS) { set_err(err, errlen, "n_colors is 1 .. 4096"); return FIN_ELIMIT; }
    if (max_iters == 0) { set_err(err, errlen, "max_iters is 1 .. 100000"); return FIN_EINVAL; }
    if (max_iters > FIN_AB_MAX_ITERS) { set_err(err, errlen, "max_iters is 1 .. 100000"); return FIN_ELIMIT; }
    if (!(tol >= 0.0)) { set_err(err, errlen, "tol is a number >= 0"); return FIN_EINVAL; }
    if (lengths)
        for (uint32_t c = 0; c < n_colors; c++)
            if (!(lengths[c] > 0.0) || !std::isfinite(lengths[c])) { set_err(err, errlen, "the length of colour " + std::to_string(c) + " is not a finite positive number"); return FIN_EINVAL; }
    return FIN_OK;
}
static void ab_empty(uint32_t n_colors, double* alpha_out, fin_abundance_info* info, uint64_t n_unaligned) {
    for (uint32_t c = 0; c < n_colors; c++) alpha_out[c] = 0.0;
    if (info) { *info = fin_abundance_info(); info->n_unaligned = n_unaligned; info->converged = 1; }
}

// the dense class list of an accumulator and the buffers of the estimates over it: what fin_eqclasses_abundance and fin_eqclasses_bootstrap prepare alike
struct AbPrep {
    AbBufs bufs;
    uint64_t ctr[8] = {0};
    uint64_t C = 0, N = 0;                  // classes; the aligned reads
    uint32_t W = 0, nc = 0, ab_chunk = 0, max_iters = 0;
    size_t padded = 0;
    uint64_t *d_rows = nullptr, *d_rowsT = nullptr, *d_reads = nullptr;
    double *d_len = nullptr, *d_alpha = nullptr, *d_x = nullptr, *d_q = nullptr, *d_part = nullptr, *d_ll = nullptr, *d_chg = nullptr, *d_trace = nullptr;
    FinAbState* d_state = nullptr;
    uint32_t* d_ok = nullptr;
    std::vector<double> host;               // len (1 behind n_colors) | alpha | x, 64 W each
};
// under the accumulator's lock, on its device: the wait and the counters, the flag check, the compaction, the gather and the transpose, the buffers.  C = 0 on
// FIN_OK: no classes, nothing was allocated for an estimate.  `nomem`: what FIN_ENOMEM says
static int ab_prepare(fin_eqclasses* e, const double* lengths, uint32_t max_iters, const char* nomem_msg, AbPrep& P, char* err, size_t errlen) {
    if (const int wrc = e->pend.wait(err, errlen)) return wrc;
    HIPCHK(hipMemcpy(P.ctr, ec_ctr(e), sizeof P.ctr, hipMemcpyDeviceToHost));
    if (const int frc = ec_flagged(e, P.ctr, err, errlen)) return frc;
    const uint32_t W = e->words, nc = e->n_colors, nb = fin_ec_blocks((uint32_t)e->slots), ab_chunk = (uint32_t)optv(e->idx, O_ab_chunk);
    P.W = W; P.nc = nc; P.ab_chunk = ab_chunk; P.max_iters = max_iters;
    // (beside the table: the dense rows and reads, 8 C (W + 1) bytes, their word-major copy, 8 C W, and 8 (C + n_chunks 64 W) of q and partials)
    const auto nomem = [&] { set_err(err, errlen, nomem_msg); return FIN_ENOMEM; };
    // the download's compaction: the occupied slots counted per block, scanned, gathered -- the rows stay on the device
    const size_t off_bytes = (size_t)nb * 8 + 8;
    void* const d_tmp = P.bufs.get(off_bytes + (size_t)nb * 4);
    if (!d_tmp) return nomem();
    uint64_t* const d_off = (uint64_t*)d_tmp; uint64_t* const d_total = d_off + nb; uint32_t* const d_sum = (uint32_t*)((char*)d_tmp + off_bytes);
    int rc = fin_launch_ec_occupied(ec_tags(e), (uint32_t)e->slots, d_sum, d_off, d_total, nullptr);
    if (rc != 0) { set_err(err, errlen, std::string("compaction of the equivalence classes: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    uint64_t C = 0;
    HIPCHK(hipMemcpy(&C, d_total, 8, hipMemcpyDeviceToHost));
    if (C == 0) return FIN_OK;
    if (C > e->max_classes) { set_err(err, errlen, "more than max_classes distinct rows"); return FIN_ELIMIT; }   // (the flags said otherwise: never)
    P.N = P.ctr[0] - P.ctr[1];              // the aligned reads: every row added is unaligned or in a class
    uint32_t cpb, n_ll, chunk, n_chunks;
    fin_ab_geometry(C, W, ab_chunk, &cpb, &n_ll, &chunk, &n_chunks);
    const size_t padded = (size_t)64 * W;
    P.padded = padded;
    P.d_rows = (uint64_t*)P.bufs.get((size_t)C * (W + 1) * 8);
    P.d_rowsT = W > 1 ? (uint64_t*)P.bufs.get((size_t)C * W * 8) : P.d_rows;
    // doubles: len | alpha | x | q | part | ll_part | blk_chg | trace, then the state and blk_ok
    const size_t n_dbl = 3 * padded + (size_t)C + (size_t)n_chunks * padded + n_ll + 64 + max_iters;
    double* const d_dbl = (double*)P.bufs.get(n_dbl * 8 + sizeof(FinAbState) + 64 * 4);
    if (!P.d_rows || !P.d_rowsT || !d_dbl) return nomem();
    P.d_reads = P.d_rows + (size_t)C * W;
    P.d_len = d_dbl; P.d_alpha = P.d_len + padded; P.d_x = P.d_alpha + padded; P.d_q = P.d_x + padded;
    P.d_part = P.d_q + C; P.d_ll = P.d_part + (size_t)n_chunks * padded; P.d_chg = P.d_ll + n_ll; P.d_trace = P.d_chg + 64;
    P.d_state = (FinAbState*)(P.d_trace + max_iters); P.d_ok = (uint32_t*)(P.d_state + 1);
    rc = fin_launch_ec_gather(ec_tags(e), ec_counts(e), ec_rows(e), (uint32_t)e->slots, W, d_off, P.d_rows, P.d_reads, nullptr);
    if (rc == 0 && W > 1) rc = fin_launch_ab_transpose(P.d_rows, C, W, P.d_rowsT, nullptr);
    if (rc != 0) { set_err(err, errlen, std::string("abundance kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    P.host.assign(3 * padded, 0.0);
    for (size_t c = 0; c < padded; c++) P.host[c] = c < nc && lengths ? lengths[c] : 1.0;
    P.C = C;
    return FIN_OK;
}
// one estimate over the prepared list: the counts `d_counts` (the list's reads, or a replicate's) and their total, from alpha0 = n_total / n_colors with a fresh
// state; *st: the device's state word when it stopped
static int ab_estimate(AbPrep& P, const uint64_t* d_counts, uint64_t n_total, double tol, FinAbState* st_out, char* err, size_t errlen) {
    const size_t padded = P.padded;
    const uint32_t nc = P.nc, max_iters = P.max_iters;
    for (uint32_t c = 0; c < nc; c++) { P.host[padded + c] = (double)n_total / (double)nc; P.host[2 * padded + c] = P.host[padded + c] / P.host[c]; }
    HIPCHK(hipMemcpy(P.d_len, P.host.data(), P.host.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(P.d_state, 0, sizeof(FinAbState) + 64 * 4));
    FinAbState st = FinAbState();
    for (uint32_t t = 0; t < max_iters && !st.done;) {
        const uint32_t t1 = std::min(max_iters, t + FIN_AB_GROUP);
        for (; t < t1; t++) {
            const int rc = fin_launch_ab_iteration(P.d_state, P.d_rows, P.d_rowsT, d_counts, P.C, P.W, nc, P.ab_chunk, P.d_len, (double)n_total, tol, P.d_alpha, P.d_x, P.d_q,
                                                   P.d_part, P.d_ll, P.d_ok, P.d_chg, t, P.d_trace, nullptr);
            if (rc != 0) { set_err(err, errlen, std::string("abundance kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
        }
        HIPCHK(hipMemcpy(&st, P.d_state, 8, hipMemcpyDeviceToHost));   // {done, iters}: the copy waits for the group
    }
    HIPCHK(hipMemcpy(&st, P.d_state, sizeof st, hipMemcpyDeviceToHost));
    if (st.iters == 0 || st.iters > max_iters) { set_err(err, errlen, "abundance kernels: the iteration count on the device is out of range"); return FIN_ENODEV; }
    *st_out = st;
    return FIN_OK;
}
// the point estimate's outputs
static int ab_point(AbPrep& P, double tol, double* alpha_out, double* loglik_trace, fin_abundance_info* info, char* err, size_t errlen) {
    FinAbState st;
    if (const int rc = ab_estimate(P, P.d_reads, P.N, tol, &st, err, errlen)) return rc;
    HIPCHK(hipMemcpy(alpha_out, P.d_alpha, (size_t)P.nc * 8, hipMemcpyDeviceToHost));
    if (loglik_trace) HIPCHK(hipMemcpy(loglik_trace, P.d_trace, (size_t)st.iters * 8, hipMemcpyDeviceToHost));
    if (info) {
        info->n_classes = P.C; info->n_reads = P.N; info->n_unaligned = P.ctr[1];
        info->iters = st.iters; info->converged = st.done ? 1u : 0u;
        info->loglik = st.loglik; info->max_change = st.max_change;
    }
    return FIN_OK;
}

int fin_eqclasses_abundance(fin_eqclasses* e, const double* lengths, uint32_t max_iters, double tol, double* alpha_out, double* loglik_trace, fin_abundance_info* info,
                            char* err, size_t errlen) {
    if (!e || !alpha_out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int arc = ab_check_args(e->n_colors, lengths, max_iters, tol, err, errlen)) return arc;
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    AbPrep P;
    if (const int prc = ab_prepare(e, lengths, max_iters, "out of device memory (abundances from the equivalence classes: beside the table, 16 W + 16 bytes per class and up to 32 MB of partial sums)", P, err, errlen)) return prc;
    if (P.C == 0) { ab_empty(e->n_colors, alpha_out, info, P.ctr[1]); return FIN_OK; }
    return ab_point(P, tol, alpha_out, loglik_trace, info, err, errlen);
}

// ---- bootstrap replicates of the estimate (fin_bootstrap.hip, fin_bootrng.h) ------------------------------------------------
int fin_bootstrap_check(uint64_t n_reads, uint32_t n_boot, char* err, size_t errlen) {
    if (n_boot == 0) { set_err(err, errlen, "n_boot is 1 .. 4096"); return FIN_EINVAL; }
    if (n_boot > FIN_BOOT_MAX) { set_err(err, errlen, "n_boot is 1 .. 4096"); return FIN_ELIMIT; }
    if (n_reads > FIN_BOOT_MAX_DRAWS / n_boot) {
        set_err(err, errlen, "N x n_boot = " + std::to_string(n_reads) + " reads x " + std::to_string(n_boot) + " replicates is more than 2^38 draws in one call");
        return FIN_ELIMIT;
    }
    return FIN_OK;
}

int fin_eqclasses_bootstrap(fin_eqclasses* e, const double* lengths, uint32_t max_iters, double tol, uint32_t n_boot, uint64_t seed, double* alpha_out,
                            fin_abundance_info* info, double* boot_alpha_out, uint64_t* boot_reads_out, uint32_t* boot_iters_out, uint8_t* boot_converged_out, char* err,
                            size_t errlen) {
    if (!e || !alpha_out || !boot_alpha_out || !boot_reads_out || !boot_iters_out || !boot_converged_out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int arc = ab_check_args(e->n_colors, lengths, max_iters, tol, err, errlen)) return arc;
    if (const int brc = fin_bootstrap_check(0, n_boot, err, errlen)) return brc;
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::mutex> g(e->mu);
    AbPrep P;
    static const char* const nomem_msg = "out of device memory (bootstrap of the abundances: beside the table, 16 W + 40 bytes per class and up to 32 MB of partial sums)";
    if (const int prc = ab_prepare(e, lengths, max_iters, nomem_msg, P, err, errlen)) return prc;
    const uint32_t nc = P.nc;
    const auto empty_replicate = [&](uint32_t b) {
        for (uint32_t c = 0; c < nc; c++) boot_alpha_out[(size_t)b * nc + c] = 0.0;
        boot_reads_out[b] = 0; boot_iters_out[b] = 0; boot_converged_out[b] = 1;
    };
    if (P.C == 0) {
        ab_empty(nc, alpha_out, info, P.ctr[1]);
        for (uint32_t b = 0; b < n_boot; b++) empty_replicate(b);
        return FIN_OK;
    }
    if (const int brc = fin_bootstrap_check(P.N, n_boot, err, errlen)) return brc;
    const uint64_t C = P.C;
    // hash | prefix | counts, then the N_b word and the slab total: 24 bytes per class (the slabs, uint32[C], lie where the counts will)
    uint64_t* const d_boot = (uint64_t*)P.bufs.get(((size_t)3 * C + 2) * 8);
    if (!d_boot) { set_err(err, errlen, nomem_msg); return FIN_ENOMEM; }
    uint64_t* const d_hash = d_boot; uint64_t* const d_pref = d_hash + C; uint64_t* const d_counts = d_pref + C; uint64_t* const d_nb = d_counts + C; uint64_t* const d_S = d_nb + 1;
    if (const int rc = ab_point(P, tol, alpha_out, nullptr, info, err, errlen)) return rc;
    int rc = fin_launch_ab_rowhash(P.d_rows, C, P.W, d_hash, nullptr);
    if (rc == 0) rc = fin_launch_ab_slabs(P.d_reads, C, (uint32_t*)d_counts, d_pref, d_S, nullptr);
    if (rc != 0) { set_err(err, errlen, std::string("bootstrap kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    uint64_t S = 0;
    HIPCHK(hipMemcpy(&S, d_S, 8, hipMemcpyDeviceToHost));
    if (S == 0 || S > P.N / FIN_BOOT_SLAB + C) { set_err(err, errlen, "bootstrap kernels: the slab count on the device is out of range"); return FIN_ENODEV; }
    for (uint32_t b = 0; b < n_boot; b++) {
        HIPCHK(hipMemsetAsync(d_counts, 0, ((size_t)C + 1) * 8, nullptr));
        rc = fin_launch_ab_resample(d_hash, P.d_reads, d_pref, C, S, seed, b, d_counts, d_nb, nullptr);
        if (rc != 0) { set_err(err, errlen, std::string("bootstrap kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
        uint64_t n_b = 0;
        HIPCHK(hipMemcpy(&n_b, d_nb, 8, hipMemcpyDeviceToHost));
        if (n_b == 0) { empty_replicate(b); continue; }
        FinAbState st;
        if (const int erc = ab_estimate(P, d_counts, n_b, tol, &st, err, errlen)) return erc;
        HIPCHK(hipMemcpy(boot_alpha_out + (size_t)b * nc, P.d_alpha, (size_t)nc * 8, hipMemcpyDeviceToHost));
        boot_reads_out[b] = n_b; boot_iters_out[b] = st.iters; boot_converged_out[b] = st.done ? 1 : 0;
    }
    return FIN_OK;
}

// host twin: the definition over the classes in the order given.  Sums in fixed blocks, whatever the number of threads: d_j over the row's bits in ascending order,
// ll over blocks of 4096 classes and then over the blocks, S_c over chunks of classes (the device's automatic chunk) and then over the chunks
int fin_classes_abundance(const uint64_t* class_rows, const uint64_t* class_reads, uint64_t n_classes, uint32_t n_colors, const double* lengths, uint32_t max_iters,
                          double tol, double* alpha_out, double* loglik_trace, fin_abundance_info* info, int n_threads) {
    if (const int arc = ab_check_args(n_colors, lengths, max_iters, tol, nullptr, 0)) return arc;
    if ((n_classes && (!class_rows || !class_reads)) || !alpha_out) return FIN_EINVAL;
    if (n_classes > (1ull << 26)) return FIN_ELIMIT;
    const uint32_t W = (n_colors + 63u) / 64u;
    const uint64_t stray = (n_colors & 63u) ? ~0ull << (n_colors & 63u) : 0ull;
    const int64_t C = (int64_t)n_classes;
    uint64_t N = 0;
    for (int64_t j = 0; j < C; j++) {
        const uint64_t* row = class_rows + (size_t)j * W;
        bool ne = false;
        for (uint32_t w = 0; w < W; w++) if (row[w]) ne = true;
        if ((row[W - 1] & stray) || !ne || class_reads[j] == 0) return FIN_EINVAL;   // a class is a non-empty set with at least one read
        N += class_reads[j];
    }
    if (C == 0) { ab_empty(n_colors, alpha_out, info, 0); return FIN_OK; }
    const int T = n_threads > 0 ? n_threads : fin_host_threads();
    uint32_t cpb, n_ll, chunk, n_chunks;
    fin_ab_geometry(n_classes, W, 0, &cpb, &n_ll, &chunk, &n_chunks);
    const int64_t LB = 4096, n_lb = (C + LB - 1) / LB;
    std::vector<double> alpha(n_colors, (double)N / (double)n_colors), x(n_colors), q((size_t)C), ll_blk((size_t)n_lb), part((size_t)n_chunks * n_colors);
    uint32_t iters = 0, converged = 0;
    double ll = 0.0, chg = 0.0;
    for (uint32_t t = 0; t < max_iters && !converged; t++) {
        for (uint32_t c = 0; c < n_colors; c++) x[c] = alpha[c] / (lengths ? lengths[c] : 1.0);
#pragma omp parallel for num_threads(T) schedule(static)
        for (int64_t b = 0; b < n_lb; b++) {
            double s = 0.0;
            for (int64_t j = b * LB; j < std::min(C, (b + 1) * LB); j++) {
                const uint64_t* row = class_rows + (size_t)j * W;
                double d = 0.0;
                for (uint32_t w = 0; w < W; w++)
                    for (uint64_t m = row[w]; m; m &= m - 1) d += x[64u * w + (uint32_t)__builtin_ctzll(m)];
                const double n = (double)class_reads[j];
                q[(size_t)j] = d > 0.0 ? n / d : 0.0;
                if (d > 0.0) s += n * std::log(d / (double)N);
            }
            ll_blk[(size_t)b] = s;
        }
        ll = 0.0;
        for (int64_t b = 0; b < n_lb; b++) ll += ll_blk[(size_t)b];
#pragma omp parallel for num_threads(T) schedule(static)
        for (int64_t k = 0; k < (int64_t)n_chunks; k++) {
            double* const p = part.data() + (size_t)k * n_colors;
            for (uint32_t c = 0; c < n_colors; c++) p[c] = 0.0;
            for (int64_t j = k * (int64_t)chunk; j < std::min(C, (k + 1) * (int64_t)chunk); j++) {
                const uint64_t* row = class_rows + (size_t)j * W;
                for (uint32_t w = 0; w < W; w++)
                    for (uint64_t m = row[w]; m; m &= m - 1) p[64u * w + (uint32_t)__builtin_ctzll(m)] += q[(size_t)j];
            }
        }
        bool ok = true;
        chg = 0.0;
        for (uint32_t c = 0; c < n_colors; c++) {
            double S = 0.0;
            for (uint32_t k = 0; k < n_chunks; k++) S += part[(size_t)k * n_colors + c];
            const double a1 = x[c] * S, scale = a1 > 1.0 ? a1 : 1.0, diff = std::fabs(a1 - alpha[c]);
            if (!(diff <= tol * scale)) ok = false;
            if (diff / scale > chg) chg = diff / scale;
            alpha[c] = a1;
        }
        if (loglik_trace) loglik_trace[t] = ll;
        iters = t + 1;
        if (ok) converged = 1;
    }
    for (uint32_t c = 0; c < n_colors; c++) alpha_out[c] = alpha[c];
    if (info) {
        info->n_classes = n_classes; info->n_reads = N; info->n_unaligned = 0;
        info->iters = iters; info->converged = converged; info->loglik = ll; info->max_change = chg;
    }
    return FIN_OK;
}

// host twin of the resample: the exact counts of replicate b, in the order given (which does not matter).  The device's slabs, a slab per loop step, summed
// into the class with integer atomics: the result does not depend on the threads
int fin_classes_resample(const uint64_t* class_rows, const uint64_t* class_reads, uint64_t n_classes, uint32_t n_colors, uint64_t seed, uint32_t b, uint64_t* counts_out,
                         int n_threads) {
    if (n_colors == 0 || n_colors > FIN_MAX_COLORS || b >= FIN_BOOT_MAX || n_classes > (1ull << 26)) return FIN_ELIMIT;
    if (n_classes && (!class_rows || !class_reads || !counts_out)) return FIN_EINVAL;
    const uint32_t W = (n_colors + 63u) / 64u;
    std::vector<uint64_t> h((size_t)n_classes), pref((size_t)n_classes + 1, 0);
    for (uint64_t j = 0; j < n_classes; j++) {
        if (class_reads[j] >= (1ull << 40)) return FIN_ELIMIT;
        uint64_t x = 0;
        for (uint32_t w = 0; w < W; w++) x ^= ec_word_hash(class_rows[(size_t)j * W + w], w);
        h[(size_t)j] = x;
        pref[(size_t)j + 1] = pref[(size_t)j] + (class_reads[j] + (FIN_BOOT_SLAB - 1u)) / FIN_BOOT_SLAB;
        counts_out[j] = 0;
    }
    const int64_t S = (int64_t)pref[(size_t)n_classes];
    const int T = n_threads > 0 ? n_threads : fin_host_threads();
#pragma omp parallel for num_threads(T) schedule(static)
    for (int64_t s = 0; s < S; s++) {
        const size_t j = (size_t)(std::upper_bound(pref.begin(), pref.end(), (uint64_t)s) - pref.begin()) - 1;   // the last j with pref[j] <= s
        const uint64_t n = class_reads[j], i0 = ((uint64_t)s - pref[j]) * (FIN_BOOT_SLAB / 4u), i1 = std::min((n + 3u) / 4u, i0 + FIN_BOOT_SLAB / 4u);
        uint64_t sum = 0;
        for (uint64_t i = i0; i < i1; i++) sum += fin_boot_block_sum(h[j], i, n, b, seed);
        if (sum) __atomic_fetch_add(counts_out + j, sum, __ATOMIC_RELAXED);
    }
    return FIN_OK;
}

// host twin of fin_eqclasses_bootstrap: the point estimate over the classes, and for every replicate fin_classes_abundance over its non-zero classes in the
// order given
int fin_classes_bootstrap(const uint64_t* class_rows, const uint64_t* class_reads, uint64_t n_classes, uint32_t n_colors, const double* lengths, uint32_t max_iters,
                          double tol, uint32_t n_boot, uint64_t seed, double* alpha_out, fin_abundance_info* info, double* boot_alpha_out, uint64_t* boot_reads_out,
                          uint32_t* boot_iters_out, uint8_t* boot_converged_out, int n_threads) {
    if (const int arc = ab_check_args(n_colors, lengths, max_iters, tol, nullptr, 0)) return arc;
    if (!boot_alpha_out || !boot_reads_out || !boot_iters_out || !boot_converged_out) return FIN_EINVAL;
    if (const int brc = fin_bootstrap_check(0, n_boot, nullptr, 0)) return brc;
    fin_abundance_info point;
    if (const int rc = fin_classes_abundance(class_rows, class_reads, n_classes, n_colors, lengths, max_iters, tol, alpha_out, nullptr, &point, n_threads)) return rc;
    if (info) *info = point;
    if (const int brc = fin_bootstrap_check(point.n_reads, n_boot, nullptr, 0)) return brc;
    const uint32_t W = (n_colors + 63u) / 64u;
    std::vector<uint64_t> counts((size_t)n_classes), rows, reads;
    for (uint32_t b = 0; b < n_boot; b++) {
        if (const int rc = fin_classes_resample(class_rows, class_reads, n_classes, n_colors, seed, b, counts.data(), n_threads)) return rc;
        rows.clear(); reads.clear();
        uint64_t n_b = 0;
        for (uint64_t j = 0; j < n_classes; j++)
            if (counts[(size_t)j]) {
                rows.insert(rows.end(), class_rows + (size_t)j * W, class_rows + (size_t)j * W + W);
                reads.push_back(counts[(size_t)j]);
                n_b += counts[(size_t)j];
            }
        fin_abundance_info bi;
        if (const int rc = fin_classes_abundance(rows.data(), reads.data(), reads.size(), n_colors, lengths, max_iters, tol, boot_alpha_out + (size_t)b * n_colors, nullptr, &bi,
                                                 n_threads)) return rc;
        boot_reads_out[b] = n_b; boot_iters_out[b] = bi.iters; boot_converged_out[b] = bi.converged ? 1 : 0;
    }
    return FIN_OK;
}

// ---- breadth of coverage over the unitig text (fin_cover.hip) -------------------------------------------------------------------------
struct fin_cover : fin_acc {
    uint64_t n_unitigs = 0, total_len = 0, n_words = 0;
    const uint32_t* d_ends = nullptr;   // the replica's ends_p
    void* d_bits = nullptr;             // uint64[n_words], then the flag word (fin_launch_cover_add)
    void* d_covered = nullptr;          // uint64[n_unitigs]: fin_cover_download's popcounts
    std::mutex count_mu;                // one download at a time counts into d_covered
};
static uint32_t* cover_flags(const fin_cover* c) { return (uint32_t*)((uint64_t*)c->d_bits + c->n_words); }

void fin_cover_free(fin_cover* c) {
    if (!acc_free_open(c)) return;
    (void)hipFree(c->d_bits); (void)hipFree(c->d_covered);
    delete c;
}

int fin_cover_create(const fin_index* idx, int device, fin_cover** out, char* err, size_t errlen) {
    if (!idx || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    *out = nullptr;
    const fin_index::Replica* rep = nullptr;
    if (const int orc = acc_create_open(idx, device, &rep, err, errlen)) return orc;
    fin_cover* c = acc_new<fin_cover>(idx, device, err, errlen);
    if (!c) return FIN_ENOMEM;
    c->n_unitigs = idx->n_unitigs; c->total_len = idx->total_len; c->n_words = (idx->total_len + 63) / 64; c->d_ends = rep->dev.ends;
    if (const int arc = acc_alloc_zero(c, &c->d_bits, c->n_words * 8 + 8, c->n_words * 8 + 8, "out of device memory (coverage bitmap)", fin_cover_free, err, errlen)) return arc;
    if (c->n_unitigs && hipMalloc(&c->d_covered, c->n_unitigs * 8) != hipSuccess) { (void)hipGetLastError(); c->d_covered = nullptr; fin_cover_free(c); set_err(err, errlen, "out of device memory (covered counts)"); return FIN_ENOMEM; }
    *out = c;
    return FIN_OK;
}

int fin_cover_reset(fin_cover* c, void* hip_stream) {
    return acc_reset(c, hip_stream, c ? c->d_bits : nullptr, c ? c->n_words * 8 + 8 : 0);
}

void* fin_cover_device_bits(const fin_cover* c) { return c ? c->d_bits : nullptr; }

int fin_batch_add_cover(fin_batch* b, fin_cover* c, void* hip_stream, char* err, size_t errlen) {
    if (!b || !c) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    hipStream_t st = (hipStream_t)hip_stream;
    if (const int orc = acc_add_open(b, c, st, err, errlen)) return orc;
    const int rc = fin_launch_cover_add(b->last_frec ? b->d_frec : nullptr, (const uint64_t*)b->d_out_offs, b->d_out, (uint32_t)b->n_reads, b->n_kmers, b->dev.k, c->d_ends,
                                        (uint32_t)c->n_unitigs, c->total_len, c->d_bits, cover_flags(c), b->d_ovf_count, b->last_ovf_cap,
                                        (uint32_t)optv(b->idx, O_cover_probe), st);
    return acc_add_close(c, st, rc, "cover kernel: ", err, errlen);
}

// covered[] of the bitmap as it stands, into c->d_covered on the null stream (with count_mu held; n_unitigs > 0): fin_cover_download's and fin_colors_coverage's
static int cover_count(fin_cover* c, char* err, size_t errlen) {
    const int rc = fin_launch_cover_count(c->d_bits, c->d_ends, (uint32_t)c->n_unitigs, c->total_len, c->d_covered, nullptr);
    if (rc != 0) { set_err(err, errlen, std::string("cover count kernel: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    return FIN_OK;
}

int fin_cover_download(fin_cover* c, uint64_t* bits_out, uint64_t* covered_out, uint64_t* total_covered, char* err, size_t errlen) {
    if (!c) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int orc = acc_download_open(c, cover_flags(c), "a step whose overflow list overran was added: it has no results, nothing of it was set (reset the accumulator)",
                                          "a pair with a unitig number or a position outside the index was met (not set)", err, errlen)) return orc;
    if (bits_out && c->n_words) HIPCHK(hipMemcpy(bits_out, c->d_bits, c->n_words * 8, hipMemcpyDeviceToHost));
    if (covered_out || total_covered) {
        std::vector<uint64_t> tmp;
        uint64_t* const dst = dst_or_tmp(covered_out, tmp, (size_t)c->n_unitigs);
        if (c->n_unitigs) {
            std::lock_guard<std::mutex> g(c->count_mu);
            if (const int rc = cover_count(c, err, errlen)) return rc;
            HIPCHK(hipMemcpy(dst, c->d_covered, c->n_unitigs * 8, hipMemcpyDeviceToHost));   // (the null stream: behind the kernel)
        }
        if (total_covered) *total_covered = sum_of(dst, (size_t)c->n_unitigs, [](uint64_t v) { return v; });
    }
    return FIN_OK;
}

// ---- per-position depth over the unitig text (fin_depth.hip) ---------------------------------------------------------------------------
struct fin_depth : fin_acc {
    uint64_t n_unitigs = 0, total_len = 0;
    const uint32_t* d_ends = nullptr;   // the replica's ends_p
    void* d_diff = nullptr;             // int32[total_len + 1], the difference array, then the flag word (fin_launch_depth_add)
    // fin_depth_download's: made by the first download, kept
    uint32_t* d_stage = nullptr;        // uint32[stage_len]: one chunk's depths
    uint32_t* d_tile = nullptr;         // uint32[fin_depth_max_chunk_tiles()]: the chunk's tile sums, then the carry word
    void* d_stats = nullptr;            // fin_depth_stat[n_unitigs]
    void* d_hist = nullptr;             // fin_depth_histogram's uint64[FIN_DEPTH_HIST_MAX_BINS]: made by the first call, kept
    uint64_t stage_len = 0;
    std::mutex scan_mu;                 // one download at a time scans through the staging buffer
};
static_assert(sizeof(fin_depth_stat) == 16 && sizeof(FinDepthStat) == 16, "fin_depth_stat is 16 bytes on both sides");
static uint32_t* depth_flags(const fin_depth* d) { return (uint32_t*)((int32_t*)d->d_diff + d->total_len + 1); }
static size_t depth_bytes(const fin_depth* d) { return (size_t)(d->total_len + 2) * 4; }

void fin_depth_free(fin_depth* d) {
    if (!acc_free_open(d)) return;
    (void)hipFree(d->d_diff); (void)hipFree(d->d_stage); (void)hipFree(d->d_tile); (void)hipFree(d->d_stats); (void)hipFree(d->d_hist);
    delete d;
}

int fin_depth_create(const fin_index* idx, int device, fin_depth** out, char* err, size_t errlen) {
    if (!idx || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    *out = nullptr;
    const fin_index::Replica* rep = nullptr;
    if (const int orc = acc_create_open(idx, device, &rep, err, errlen)) return orc;
    fin_depth* d = acc_new<fin_depth>(idx, device, err, errlen);
    if (!d) return FIN_ENOMEM;
    d->n_unitigs = idx->n_unitigs; d->total_len = idx->total_len; d->d_ends = rep->dev.ends;
    if (const int arc = acc_alloc_zero(d, &d->d_diff, depth_bytes(d), depth_bytes(d), "out of device memory (depth difference array)", fin_depth_free, err, errlen)) return arc;
    *out = d;
    return FIN_OK;
}

int fin_depth_reset(fin_depth* d, void* hip_stream) {
    return acc_reset(d, hip_stream, d ? d->d_diff : nullptr, d ? depth_bytes(d) : 0);
}

void* fin_depth_device_diff(const fin_depth* d) { return d ? d->d_diff : nullptr; }

int fin_batch_add_depth(fin_batch* b, fin_depth* d, void* hip_stream, char* err, size_t errlen) {
    if (!b || !d) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    hipStream_t st = (hipStream_t)hip_stream;
    if (const int orc = acc_add_open(b, d, st, err, errlen)) return orc;
    const int rc = fin_launch_depth_add(b->last_frec ? b->d_frec : nullptr, (const uint64_t*)b->d_out_offs, b->d_out, (uint32_t)b->n_reads, b->n_kmers, b->dev.k, d->d_ends,
                                        (uint32_t)d->n_unitigs, d->total_len, d->d_diff, depth_flags(d), b->d_ovf_count, b->last_ovf_cap, st);
    return acc_add_close(d, st, rc, "depth kernel: ", err, errlen);
}

// the prefix sum of the difference array as it stands, a chunk at a time through the staging buffer on the null stream (with scan_mu held; total_len and
// n_unitigs > 0): every chunk's depths to depth_out (may be null), the per-unitig statistics under min_depth into d->d_stats (want_stats), and each_chunk (may be
// empty) called on every chunk once it is staged.  fin_depth_download's, fin_colors_coverage's and the depth histograms'
typedef std::function<int(uint64_t base, uint64_t n)> depth_chunk_fn;   // what else is made of a staged chunk: launches on the null stream, a hipError_t as int
static int depth_scan(fin_depth* d, uint32_t min_depth, uint32_t* depth_out, bool want_stats, char* err, size_t errlen, const depth_chunk_fn& each_chunk = nullptr) {
    // the prefix sum, a chunk of the difference array at a time through one staging buffer: no second array of total_len entries on the device
    const uint32_t dbg = (uint32_t)optv(d->idx, O_debug_depth_tile);
    const uint32_t tile = dbg ? dbg : fin_depth_max_tile(), chunk_tiles = dbg ? 64u : fin_depth_max_chunk_tiles();
    const uint64_t chunk = (uint64_t)tile * chunk_tiles;
    if (!d->d_stage) {
        d->stage_len = std::min<uint64_t>((uint64_t)fin_depth_max_tile() * fin_depth_max_chunk_tiles(), d->total_len);
        if (hipMalloc((void**)&d->d_stage, (size_t)d->stage_len * 4) != hipSuccess) { (void)hipGetLastError(); d->d_stage = nullptr; set_err(err, errlen, "out of device memory (depth staging buffer)"); return FIN_ENOMEM; }
    }
    if (!d->d_tile && hipMalloc((void**)&d->d_tile, ((size_t)fin_depth_max_chunk_tiles() + 1) * 4) != hipSuccess) { (void)hipGetLastError(); d->d_tile = nullptr; set_err(err, errlen, "out of device memory (depth tile sums)"); return FIN_ENOMEM; }
    if (want_stats && !d->d_stats && hipMalloc(&d->d_stats, (size_t)d->n_unitigs * sizeof(fin_depth_stat)) != hipSuccess) { (void)hipGetLastError(); d->d_stats = nullptr; set_err(err, errlen, "out of device memory (depth statistics)"); return FIN_ENOMEM; }
    uint32_t* const d_carry = d->d_tile + fin_depth_max_chunk_tiles();
    HIPCHK(hipMemsetAsync(d_carry, 0, 4, nullptr));
    if (want_stats) HIPCHK(hipMemsetAsync(d->d_stats, 0, (size_t)d->n_unitigs * sizeof(fin_depth_stat), nullptr));
    for (uint64_t base = 0; base < d->total_len; base += chunk) {
        const uint64_t n = std::min<uint64_t>(chunk, d->total_len - base);
        int rc = fin_launch_depth_scan_chunk((const int32_t*)d->d_diff + base, n, tile, d->d_tile, d_carry, d->d_stage, nullptr);
        if (rc == 0 && want_stats) rc = fin_launch_depth_stats(d->d_stage, base, n, d->d_ends, (uint32_t)d->n_unitigs, min_depth, d->d_stats, nullptr);
        if (rc == 0 && each_chunk) rc = each_chunk(base, n);
        if (rc != 0) { set_err(err, errlen, std::string("depth scan kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
        if (depth_out) HIPCHK(hipMemcpy(depth_out + base, d->d_stage, (size_t)n * 4, hipMemcpyDeviceToHost));   // (the null stream: behind the kernels, and done before the next chunk is staged)
    }
    return FIN_OK;
}

int fin_depth_download(fin_depth* d, uint32_t min_depth, uint32_t* depth_out, fin_depth_stat* stats_out, uint64_t* total, char* err, size_t errlen) {
    if (!d) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int orc = acc_download_open(d, depth_flags(d), "a step whose overflow list overran was added: it has no results, nothing of it was counted (reset the accumulator)",
                                          "a pair with a unitig number or a position outside the index was met (not counted)", err, errlen)) return orc;
    if (total) *total = 0;
    const bool want_stats = stats_out || total;
    if (!depth_out && !want_stats) return FIN_OK;
    if (d->total_len == 0 || d->n_unitigs == 0) return FIN_OK;
    std::lock_guard<std::mutex> g(d->scan_mu);
    if (const int rc = depth_scan(d, min_depth, depth_out, want_stats, err, errlen)) return rc;
    if (want_stats) {
        std::vector<fin_depth_stat> tmp;
        fin_depth_stat* const dst = dst_or_tmp(stats_out, tmp, (size_t)d->n_unitigs);
        HIPCHK(hipMemcpy(dst, d->d_stats, (size_t)d->n_unitigs * sizeof(fin_depth_stat), hipMemcpyDeviceToHost));
        if (total) *total = sum_of(dst, (size_t)d->n_unitigs, [](const fin_depth_stat& s) { return s.sum; });
    }
    return FIN_OK;
}

// ---- breadth and depth of coverage per reference (fin_colcov.hip) -------------------------------------------------------------------------
static_assert(sizeof(fin_color_coverage) == 64, "fin_color_coverage is eight uint64");
int fin_colors_coverage(fin_colors* c, fin_cover* cov, fin_depth* dep, uint32_t min_depth, fin_color_coverage* out, fin_color_coverage* uncolored, char* err, size_t errlen) {
    if (!c || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (cov && (cov->idx != c->idx || cov->device != c->device)) { set_err(err, errlen, "colours and coverage bitmap belong to different indexes or devices"); return FIN_EINVAL; }
    if (dep && (dep->idx != c->idx || dep->device != c->device)) { set_err(err, errlen, "colours and depth accumulator belong to different indexes or devices"); return FIN_EINVAL; }
    if (const int drc = colors_want_dense(c, err, errlen)) return drc;   // (the projection reads bits[u * W + w])
    // the three waits, with the downloads' own codes and messages for a withheld step or a pair outside the index (nothing else happens in these calls)
    if (const int rc = fin_colors_download(c, nullptr, nullptr, err, errlen)) return rc;
    if (cov) if (const int rc = fin_cover_download(cov, nullptr, nullptr, nullptr, err, errlen)) return rc;
    if (dep) if (const int rc = fin_depth_download(dep, min_depth, nullptr, nullptr, nullptr, err, errlen)) return rc;
    const fin_index::Replica* rep = c->idx->replica_on(c->device);
    if (!rep) { set_err(err, errlen, "index is not resident on that device: call fin_index_to_device first (no CPU fallback)"); return FIN_ENODEV; }
    const size_t table = ((size_t)c->n_colors + 1) * 64;
    std::lock_guard<std::mutex> g(c->ccv_mu);
    if (!c->d_ccv && hipMalloc(&c->d_ccv, table + (size_t)c->n_unitigs + 8) != hipSuccess) { (void)hipGetLastError(); c->d_ccv = nullptr; set_err(err, errlen, "out of device memory (colour coverage table)"); return FIN_ENOMEM; }
    // covered[] and the statistics stay on the device; everything below is on the null stream, and the two locks keep a download from counting or scanning in between
    std::unique_lock<std::mutex> gc, gd;
    const bool with_cov = cov && c->n_unitigs, with_dep = dep && dep->total_len && c->n_unitigs;
    if (with_cov) {
        gc = std::unique_lock<std::mutex>(cov->count_mu);
        if (const int rc = cover_count(cov, err, errlen)) return rc;
    }
    if (with_dep) {
        gd = std::unique_lock<std::mutex>(dep->scan_mu);
        if (const int rc = depth_scan(dep, min_depth, nullptr, true, err, errlen)) return rc;
    }
    uint64_t* const d_out = (uint64_t*)c->d_ccv;
    uint64_t* const d_none = d_out + (size_t)c->n_colors * 8;
    const int rc = fin_launch_color_coverage(c->d_bits, (uint32_t)c->n_unitigs, c->words, c->n_colors, rep->dev.ends, c->idx->total_len, rep->dev.k,
                                             with_cov ? cov->d_covered : nullptr, with_dep ? dep->d_stats : nullptr, d_none + 8, (uint32_t)optv(c->idx, O_colcov_chunk), 0u,
                                             d_out, d_none, nullptr);
    if (rc != 0) { set_err(err, errlen, std::string("colour coverage kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    std::vector<fin_color_coverage> host((size_t)c->n_colors + 1);
    HIPCHK(hipMemcpy(host.data(), d_out, table, hipMemcpyDeviceToHost));   // (the null stream: behind the kernels)
    memcpy(out, host.data(), (size_t)c->n_colors * 64);
    if (uncolored) *uncolored = host[c->n_colors];
    return FIN_OK;
}

// ---- depth histograms, per index and per reference (fin_depthhist.hip) ---------------------------------------------------------------------
static int depthhist_args(uint32_t n_bins, uint32_t bin_width, char* err, size_t errlen) {
    if (n_bins == 0 || n_bins > FIN_DEPTH_HIST_MAX_BINS) { set_err(err, errlen, "n_bins is 1 .. " + std::to_string(FIN_DEPTH_HIST_MAX_BINS)); return FIN_EINVAL; }
    if (bin_width == 0) { set_err(err, errlen, "bin_width is at least 1"); return FIN_EINVAL; }
    return FIN_OK;
}
int fin_depth_histogram(fin_depth* d, uint32_t n_bins, uint32_t bin_width, uint64_t* hist_out, char* err, size_t errlen) {
    if (!d || !hist_out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int arc = depthhist_args(n_bins, bin_width, err, errlen)) return arc;
    // the wait, with the download's own codes and messages for a withheld step or a pair outside the index (nothing else happens in this call)
    if (const int rc = fin_depth_download(d, 0, nullptr, nullptr, nullptr, err, errlen)) return rc;
    if (d->total_len == 0 || d->n_unitigs == 0) { memset(hist_out, 0, (size_t)n_bins * 8); return FIN_OK; }
    const uint32_t k = d->idx->k;
    std::lock_guard<std::mutex> g(d->scan_mu);   // (d_hist is the scan's, like the staging buffer)
    if (!d->d_hist && hipMalloc(&d->d_hist, (size_t)FIN_DEPTH_HIST_MAX_BINS * 8) != hipSuccess) { (void)hipGetLastError(); d->d_hist = nullptr; set_err(err, errlen, "out of device memory (depth histogram)"); return FIN_ENOMEM; }
    HIPCHK(hipMemsetAsync(d->d_hist, 0, (size_t)n_bins * 8, nullptr));
    const int rc = depth_scan(d, 0, nullptr, false, err, errlen, [&](uint64_t base, uint64_t n) {
        return fin_launch_depth_spectrum(d->d_stage, base, n, d->d_ends, (uint32_t)d->n_unitigs, d->total_len, k, n_bins, bin_width, (uint64_t*)d->d_hist, nullptr);
    });
    if (rc) return rc;
    std::vector<uint64_t> host(n_bins);
    HIPCHK(hipMemcpy(host.data(), d->d_hist, (size_t)n_bins * 8, hipMemcpyDeviceToHost));   // (the null stream: behind the kernels)
    memcpy(hist_out, host.data(), (size_t)n_bins * 8);
    return FIN_OK;
}

int fin_colors_depth_histogram(fin_colors* c, fin_depth* dep, uint32_t n_bins, uint32_t bin_width, uint64_t* out, uint64_t* uncolored, char* err, size_t errlen) {
    if (!c || !dep || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int arc = depthhist_args(n_bins, bin_width, err, errlen)) return arc;
    if (dep->idx != c->idx || dep->device != c->device) { set_err(err, errlen, "colours and depth accumulator belong to different indexes or devices"); return FIN_EINVAL; }
    if (const int drc = colors_want_dense(c, err, errlen)) return drc;   // (the projection reads bits[u * W + w])
    if (const int rc = fin_colors_download(c, nullptr, nullptr, err, errlen)) return rc;
    if (const int rc = fin_depth_download(dep, 0, nullptr, nullptr, nullptr, err, errlen)) return rc;
    const size_t cells = (size_t)c->n_colors * 2 * n_bins;
    if (dep->total_len == 0 || c->n_unitigs == 0) {
        memset(out, 0, cells * 8);
        if (uncolored) memset(uncolored, 0, (size_t)n_bins * 8);
        return FIN_OK;
    }
    const fin_index::Replica* rep = c->idx->replica_on(c->device);
    if (!rep) { set_err(err, errlen, "index is not resident on that device: call fin_index_to_device first (no CPU fallback)"); return FIN_ENODEV; }
    // unitigs per sub-range: what the table's budget holds, the option below it
    const uint64_t budget = (64ull << 20) / ((uint64_t)n_bins * 4);   // >= 16384
    const uint64_t opt = (uint64_t)optv(c->idx, O_depthhist_unitigs);
    const uint32_t per = (uint32_t)std::min<uint64_t>(opt ? std::min(opt, budget) : budget, c->n_unitigs);
    // one buffer kept on the colours: the table and the uncoloured histogram behind it, the class kernel's scratch, the class bytes, the sub-range's table
    const size_t out_bytes = (cells + n_bins) * 8, cls_bytes = ((size_t)c->n_unitigs + 15) / 16 * 16, need = out_bytes + 64 + cls_bytes + (size_t)per * n_bins * 4;
    std::lock_guard<std::mutex> gh(c->dh_mu);
    if (c->dh_bytes < need) {
        (void)hipFree(c->d_dh); c->d_dh = nullptr; c->dh_bytes = 0;
        if (hipMalloc(&c->d_dh, need) != hipSuccess) { (void)hipGetLastError(); c->d_dh = nullptr; set_err(err, errlen, "out of device memory (colour depth histograms)"); return FIN_ENOMEM; }
        c->dh_bytes = need;
    }
    uint64_t* const o = (uint64_t*)c->d_dh;
    uint64_t* const none8 = (uint64_t*)((char*)c->d_dh + out_bytes);
    uint8_t* const cls = (uint8_t*)c->d_dh + out_bytes + 64;
    uint32_t* const d_V = (uint32_t*)((char*)c->d_dh + out_bytes + 64 + cls_bytes);
    const uint32_t nu = (uint32_t)c->n_unitigs, k = rep->dev.k;
    const uint32_t* const ends = c->idx->ends.data();   // ends_p on the host: ends[u] is the start of unitig u, ends[nu] == total_len
    std::lock_guard<std::mutex> g(dep->scan_mu);
    HIPCHK(hipMemsetAsync(o, 0, out_bytes, nullptr));
    if (const int krc = fin_launch_color_classes(c->d_bits, nu, c->words, rep->dev.ends, c->idx->total_len, k, cls, none8, nullptr)) {
        set_err(err, errlen, std::string("colour class kernel: ") + hipGetErrorString((hipError_t)krc)); return FIN_ENODEV;
    }
    uint32_t u_at = 0;   // the unitig that holds the chunk's first position: chunks ascend, so does this
    const int rc = depth_scan(dep, 0, nullptr, false, err, errlen, [&](uint64_t base, uint64_t n) {
        while (u_at + 1u < nu && ends[u_at + 1u] <= base) u_at++;
        // a unitig that straddles a chunk or a sub-range seam is binned twice with partial counts, which the sums do not notice
        for (uint64_t u_lo = u_at; u_lo < nu && ends[u_lo] < base + n; u_lo += per) {
            const uint32_t u_hi = (uint32_t)std::min<uint64_t>(nu, u_lo + per);
            const uint64_t lo = std::max<uint64_t>(ends[u_lo], base) - base, hi = std::min<uint64_t>(ends[u_hi], base + n) - base;
            const int krc = fin_launch_color_depth_hist(dep->d_stage, base, n, lo, hi, rep->dev.ends, nu, c->idx->total_len, k, n_bins, bin_width, (uint32_t)u_lo, u_hi,
                                                        d_V, c->d_bits, c->words, c->n_colors, cls, 0u, o, o + cells, nullptr);
            if (krc) return krc;
        }
        return 0;
    });
    if (rc) return rc;
    std::vector<uint64_t> host(cells + n_bins);
    HIPCHK(hipMemcpy(host.data(), o, out_bytes, hipMemcpyDeviceToHost));   // (the null stream: behind the kernels)
    memcpy(out, host.data(), cells * 8);
    if (uncolored) memcpy(uncolored, host.data() + cells, (size_t)n_bins * 8);
    return FIN_OK;
}

// ---- shared k-mers between references (fin_colsim.hip) ---------------------------------------------------------------------------------------
int fin_colors_shared(fin_colors* c, fin_cover* cov, const uint64_t* weights, uint64_t* out, char* err, size_t errlen) {
    if (!c || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (cov && weights) { set_err(err, errlen, "a coverage bitmap and weights were both given: one weight per unitig and call"); return FIN_EINVAL; }
    if (cov && (cov->idx != c->idx || cov->device != c->device)) { set_err(err, errlen, "colours and coverage bitmap belong to different indexes or devices"); return FIN_EINVAL; }
    if (const int drc = colors_want_dense(c, err, errlen)) return drc;   // (the product reads bits[u * W + w])
    // the two waits, with the downloads' own codes and messages for a withheld step (nothing else happens in these calls)
    if (const int rc = fin_colors_download(c, nullptr, nullptr, err, errlen)) return rc;
    if (cov) if (const int rc = fin_cover_download(cov, nullptr, nullptr, nullptr, err, errlen)) return rc;
    const fin_index::Replica* rep = c->idx->replica_on(c->device);
    if (!rep) { set_err(err, errlen, "index is not resident on that device: call fin_index_to_device first (no CPU fallback)"); return FIN_ENODEV; }
    // the call's own buffers, freed on every way out: no result of an earlier call is there to be read
    struct Buf { void* p = nullptr; ~Buf() { (void)hipFree(p); } } d_out, d_w;
    const size_t table = (size_t)c->n_colors * c->n_colors * 8;
    if (hipMalloc(&d_out.p, table) != hipSuccess) { (void)hipGetLastError(); d_out.p = nullptr; set_err(err, errlen, "out of device memory (shared k-mer table)"); return FIN_ENOMEM; }
    const bool with_w = weights && c->n_unitigs, with_cov = cov && c->n_unitigs;
    if (with_w) {
        if (hipMalloc(&d_w.p, (size_t)c->n_unitigs * 8) != hipSuccess) { (void)hipGetLastError(); d_w.p = nullptr; set_err(err, errlen, "out of device memory (unitig weights)"); return FIN_ENOMEM; }
        HIPCHK(hipMemcpy(d_w.p, weights, (size_t)c->n_unitigs * 8, hipMemcpyHostToDevice));
    }
    // covered[] stays on the device; everything below is on the null stream, and the lock keeps a download from counting in between
    std::unique_lock<std::mutex> gc;
    if (with_cov) {
        gc = std::unique_lock<std::mutex>(cov->count_mu);
        if (const int rc = cover_count(cov, err, errlen)) return rc;
    }
    const int rc = fin_launch_color_shared(c->d_bits, (uint32_t)c->n_unitigs, c->words, c->n_colors, rep->dev.ends, c->idx->total_len, rep->dev.k,
                                           with_cov ? cov->d_covered : d_w.p, (uint32_t)optv(c->idx, O_colsim_chunk), (uint64_t*)d_out.p, nullptr);
    if (rc != 0) { set_err(err, errlen, std::string("shared k-mer kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    HIPCHK(hipMemcpy(out, d_out.p, table, hipMemcpyDeviceToHost));   // (the null stream: behind the kernels)
    return FIN_OK;
}

// ---- base pileup over the unitig text (fin_pileup.hip) -----------------------------------------------------------------------------------
struct fin_pileup : fin_acc {
    uint64_t n_unitigs = 0, total_len = 0;
    uint32_t max_mismatch = 0;
    const uint32_t* d_ends = nullptr;     // the replica's ends_p
    const uint32_t* d_concat = nullptr;   // ... and its 2-bit text
    // one allocation, zeroed by one memset: uint32 alt[total_len][4], the four counters (u64), the flag word in a 16-byte line of its own, int32 cov_diff[total_len + 1]
    void* d_buf = nullptr;
    // fin_pileup_download's and fin_pileup_call's: made by the first of them, kept
    uint32_t* d_stage = nullptr;          // uint32[stage_len]: one chunk's cover
    uint32_t* d_tile = nullptr;           // uint32[fin_depth_max_chunk_tiles()]: the chunk's tile sums, then the carry word
    uint32_t* d_blk_sum = nullptr;        // the call's per-block counts of a chunk, fin_pileup_call_blocks(call chunk) of them
    uint64_t* d_blk_off = nullptr;        // ... their offsets, then the chunk's total
    void* d_ent = nullptr;                // fin_variant[call chunk]: a chunk's entries
    uint64_t stage_len = 0;
    std::mutex scan_mu;                   // one download or call at a time scans through the staging buffers
};
static_assert(sizeof(fin_variant) == 32, "fin_variant is two 16-byte stores of the call's writing pass");
static const uint32_t PILEUP_CALL_CHUNK_TILES = 256;   // a call's chunk: at most 256 tiles of 4096 positions -- 32 MB of entries if every position were a candidate
static uint64_t* pileup_counters(const fin_pileup* p) { return (uint64_t*)((uint8_t*)p->d_buf + p->total_len * 16); }
static uint32_t* pileup_flags(const fin_pileup* p) { return (uint32_t*)((uint8_t*)p->d_buf + p->total_len * 16 + 32); }
static int32_t* pileup_diff(const fin_pileup* p) { return (int32_t*)((uint8_t*)p->d_buf + p->total_len * 16 + 48); }
static size_t pileup_bytes(const fin_pileup* p) { return (size_t)p->total_len * 16 + 48 + (size_t)(p->total_len + 1) * 4; }
static const char* const PILEUP_WITHHELD = "a step whose overflow list overran was added: it has no results, nothing of it was counted (reset the accumulator)";
static const char* const PILEUP_OUTSIDE = "a slot or a record outside the index was met (not counted)";

void fin_pileup_free(fin_pileup* p) {
    if (!acc_free_open(p)) return;
    (void)hipFree(p->d_buf); (void)hipFree(p->d_stage); (void)hipFree(p->d_tile); (void)hipFree(p->d_blk_sum); (void)hipFree(p->d_blk_off); (void)hipFree(p->d_ent);
    delete p;
}

int fin_pileup_create(const fin_index* idx, int device, uint32_t max_mismatch, fin_pileup** out, char* err, size_t errlen) {
    if (!idx || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    *out = nullptr;
    if (max_mismatch > 255u) { set_err(err, errlen, "max_mismatch is 0 .. 255"); return FIN_EINVAL; }
    const fin_index::Replica* rep = nullptr;
    if (const int orc = acc_create_open(idx, device, &rep, err, errlen)) return orc;
    fin_pileup* p = acc_new<fin_pileup>(idx, device, err, errlen);
    if (!p) return FIN_ENOMEM;
    p->n_unitigs = idx->n_unitigs; p->total_len = idx->total_len; p->max_mismatch = max_mismatch; p->d_ends = rep->dev.ends; p->d_concat = rep->dev.concat;
    if (const int arc = acc_alloc_zero(p, &p->d_buf, pileup_bytes(p), pileup_bytes(p), "out of device memory (pileup: 20 bytes per indexed base)", fin_pileup_free, err, errlen)) return arc;
    *out = p;
    return FIN_OK;
}

int fin_pileup_reset(fin_pileup* p, void* hip_stream) {
    return acc_reset(p, hip_stream, p ? p->d_buf : nullptr, p ? pileup_bytes(p) : 0);
}

void* fin_pileup_device_alt(const fin_pileup* p) { return p ? p->d_buf : nullptr; }
void* fin_pileup_device_cover_diff(const fin_pileup* p) { return p ? (void*)pileup_diff(p) : nullptr; }

int fin_batch_add_pileup(fin_batch* b, fin_pileup* p, void* hip_stream, char* err, size_t errlen) {
    if (!b || !p) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    hipStream_t st = (hipStream_t)hip_stream;
    if (const int orc = acc_add_open(b, p, st, err, errlen)) return orc;
    const int rc = p->n_unitigs == 0 || p->total_len == 0 ? 0 :
        fin_launch_pileup_add(b->last_frec ? b->d_frec : nullptr, (const uint64_t*)b->d_out_offs, b->d_out, b->d_bases, (const uint64_t*)b->d_offs, (uint32_t)b->n_reads,
                              b->dev.k, p->d_ends, p->d_concat, (uint32_t)p->n_unitigs, p->total_len, p->max_mismatch, p->d_buf, pileup_diff(p), pileup_counters(p),
                              pileup_flags(p), b->d_ovf_count, b->last_ovf_cap, st);
    return acc_add_close(p, st, rc, "pileup kernel: ", err, errlen);
}

// the staging buffers of the download and the call (with scan_mu held); the tile and the chunk's tiles as fin_depth_download takes them from "debug_depth_tile"
static int pileup_stage(fin_pileup* p, bool for_call, uint32_t* tile, uint32_t* chunk_tiles, char* err, size_t errlen) {
    const uint32_t dbg = (uint32_t)optv(p->idx, O_debug_depth_tile);
    *tile = dbg ? dbg : fin_depth_max_tile(); *chunk_tiles = dbg ? 64u : fin_depth_max_chunk_tiles();
    if (for_call) *chunk_tiles = std::min(*chunk_tiles, PILEUP_CALL_CHUNK_TILES);
    auto room = [&](void** q, size_t bytes, const char* what) {
        if (*q || hipMalloc(q, bytes) == hipSuccess) return FIN_OK;
        (void)hipGetLastError(); *q = nullptr; set_err(err, errlen, what); return FIN_ENOMEM;
    };
    if (!p->d_stage) p->stage_len = std::min<uint64_t>((uint64_t)fin_depth_max_tile() * fin_depth_max_chunk_tiles(), p->total_len);
    if (const int rc = room((void**)&p->d_stage, (size_t)p->stage_len * 4, "out of device memory (pileup staging buffer)")) return rc;
    if (const int rc = room((void**)&p->d_tile, ((size_t)fin_depth_max_chunk_tiles() + 1) * 4, "out of device memory (pileup tile sums)")) return rc;
    if (!for_call) return FIN_OK;
    const uint64_t call_chunk = std::min<uint64_t>((uint64_t)fin_depth_max_tile() * PILEUP_CALL_CHUNK_TILES, p->total_len);
    const size_t nb = fin_pileup_call_blocks(call_chunk);
    if (const int rc = room((void**)&p->d_blk_sum, nb * 4, "out of device memory (pileup call)")) return rc;
    if (const int rc = room((void**)&p->d_blk_off, (nb + 1) * 8, "out of device memory (pileup call)")) return rc;
    return room(&p->d_ent, (size_t)call_chunk * sizeof(fin_variant), "out of device memory (pileup call entries)");
}

int fin_pileup_download(fin_pileup* p, uint32_t* cover_out, uint32_t* alt_out, uint64_t counters_out[4], char* err, size_t errlen) {
    if (!p) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int orc = acc_download_open(p, pileup_flags(p), PILEUP_WITHHELD, PILEUP_OUTSIDE, err, errlen)) return orc;
    if (counters_out) HIPCHK(hipMemcpy(counters_out, pileup_counters(p), 32, hipMemcpyDeviceToHost));
    if (p->total_len == 0 || p->n_unitigs == 0) return FIN_OK;
    if (alt_out) HIPCHK(hipMemcpy(alt_out, p->d_buf, (size_t)p->total_len * 16, hipMemcpyDeviceToHost));
    if (!cover_out) return FIN_OK;
    std::lock_guard<std::mutex> g(p->scan_mu);
    uint32_t tile = 0, chunk_tiles = 0;
    if (const int src = pileup_stage(p, false, &tile, &chunk_tiles, err, errlen)) return src;
    const uint64_t chunk = (uint64_t)tile * chunk_tiles;
    uint32_t* const d_carry = p->d_tile + fin_depth_max_chunk_tiles();
    HIPCHK(hipMemsetAsync(d_carry, 0, 4, nullptr));
    for (uint64_t base = 0; base < p->total_len; base += chunk) {
        const uint64_t n = std::min<uint64_t>(chunk, p->total_len - base);
        const int rc = fin_launch_depth_scan_chunk(pileup_diff(p) + base, n, tile, p->d_tile, d_carry, p->d_stage, nullptr);
        if (rc != 0) { set_err(err, errlen, std::string("pileup scan kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
        HIPCHK(hipMemcpy(cover_out + base, p->d_stage, (size_t)n * 4, hipMemcpyDeviceToHost));   // (the null stream: behind the kernels, and done before the next chunk is staged)
    }
    return FIN_OK;
}

int fin_pileup_call(fin_pileup* p, uint32_t min_alt, uint32_t min_permille, fin_variant* out, uint64_t cap, uint64_t* n_out, char* err, size_t errlen) {
    if (!p || !n_out || (cap && !out)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    *n_out = 0;
    if (const int prc = check_permille(min_permille, BAD_MIN_PERMILLE, err, errlen)) return prc;
    if (const int orc = acc_download_open(p, pileup_flags(p), PILEUP_WITHHELD, PILEUP_OUTSIDE, err, errlen)) return orc;
    if (p->total_len == 0 || p->n_unitigs == 0) return FIN_OK;
    std::lock_guard<std::mutex> g(p->scan_mu);
    uint32_t tile = 0, chunk_tiles = 0;
    if (const int src = pileup_stage(p, true, &tile, &chunk_tiles, err, errlen)) return src;
    const uint64_t chunk = (uint64_t)tile * chunk_tiles;
    uint32_t* const d_carry = p->d_tile + fin_depth_max_chunk_tiles();
    uint64_t* const d_total = p->d_blk_off + fin_pileup_call_blocks(std::min<uint64_t>((uint64_t)fin_depth_max_tile() * PILEUP_CALL_CHUNK_TILES, p->total_len));
    HIPCHK(hipMemsetAsync(d_carry, 0, 4, nullptr));
    uint64_t total = 0;
    // every chunk is counted, so that the count is the true one also when the entries do not fit; they are written only while they do
    for (uint64_t base = 0; base < p->total_len; base += chunk) {
        const uint64_t n = std::min<uint64_t>(chunk, p->total_len - base);
        const uint32_t* const alt = (const uint32_t*)p->d_buf + base * 4;
        int rc = fin_launch_depth_scan_chunk(pileup_diff(p) + base, n, tile, p->d_tile, d_carry, p->d_stage, nullptr);
        if (rc == 0) rc = fin_launch_pileup_call_count(p->d_stage, alt, n, min_alt, min_permille, p->d_blk_sum, p->d_blk_off, d_total, nullptr);
        if (rc != 0) { set_err(err, errlen, std::string("pileup call kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
        uint64_t c = 0;
        HIPCHK(hipMemcpy(&c, d_total, 8, hipMemcpyDeviceToHost));
        if (c && total + c <= cap) {
            rc = fin_launch_pileup_call_write(p->d_stage, alt, base, n, min_alt, min_permille, p->d_ends, p->d_concat, (uint32_t)p->n_unitigs, p->d_blk_off, p->d_ent, nullptr);
            if (rc != 0) { set_err(err, errlen, std::string("pileup call kernels: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
            HIPCHK(hipMemcpy(out + total, p->d_ent, (size_t)c * sizeof(fin_variant), hipMemcpyDeviceToHost));
        }
        total += c;
    }
    *n_out = total;
    if (total > cap) { set_err(err, errlen, std::to_string(total) + " candidates, room for " + std::to_string(cap)); return FIN_ELIMIT; }
    return FIN_OK;
}

// ---- fragment geometry of paired reads (fin_fragments.hip) -------------------------------------------------------------------------------
struct fin_fragments : fin_acc {
    uint64_t n_unitigs = 0;
    uint32_t n_bins = 0, bin_width = 0;
    const uint32_t* d_ends = nullptr;     // the replica's ends_p
    void* d_buf = nullptr;                // one allocation, zeroed by one memset: uint64 hist[n_bins], the seven counters (u64), the flag word
};
static_assert(sizeof(fin_fragment) == 16, "fin_fragment is one 16-byte store of the kernel");
static uint64_t* fragments_counters(const fin_fragments* f) { return (uint64_t*)f->d_buf + f->n_bins; }
static uint32_t* fragments_flags(const fin_fragments* f) { return (uint32_t*)((uint64_t*)f->d_buf + f->n_bins + 7); }
static size_t fragments_bytes(const fin_fragments* f) { return ((size_t)f->n_bins + 8) * 8; }
static int check_even_fragments(uint64_t n_reads, char* err, size_t errlen) {
    if (n_reads & 1u) { set_err(err, errlen, "fragments want interleaved mates: " + std::to_string(n_reads) + " reads are an odd number"); return FIN_EINVAL; }
    return FIN_OK;
}

void fin_fragments_free(fin_fragments* f) {
    if (!acc_free_open(f)) return;
    (void)hipFree(f->d_buf);
    delete f;
}

int fin_fragments_create(const fin_index* idx, int device, uint32_t n_bins, uint32_t bin_width, fin_fragments** out, char* err, size_t errlen) {
    if (!idx || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    *out = nullptr;
    if (n_bins == 0 || n_bins > FIN_FRAG_MAX_BINS) { set_err(err, errlen, "n_bins is 1 .. " + std::to_string(FIN_FRAG_MAX_BINS)); return FIN_EINVAL; }
    if (bin_width == 0) { set_err(err, errlen, "bin_width is at least 1"); return FIN_EINVAL; }
    const fin_index::Replica* rep = nullptr;
    if (const int orc = acc_create_open(idx, device, &rep, err, errlen)) return orc;
    fin_fragments* f = acc_new<fin_fragments>(idx, device, err, errlen);
    if (!f) return FIN_ENOMEM;
    f->n_unitigs = idx->n_unitigs; f->n_bins = n_bins; f->bin_width = bin_width; f->d_ends = rep->dev.ends;
    if (const int arc = acc_alloc_zero(f, &f->d_buf, fragments_bytes(f), fragments_bytes(f), "out of device memory (fragment histogram)", fin_fragments_free, err, errlen)) return arc;
    *out = f;
    return FIN_OK;
}

int fin_fragments_reset(fin_fragments* f, void* hip_stream) {
    return acc_reset(f, hip_stream, f ? f->d_buf : nullptr, f ? fragments_bytes(f) : 0);
}

void* fin_fragments_device_hist(const fin_fragments* f) { return f ? f->d_buf : nullptr; }

int fin_batch_add_fragments(fin_batch* b, fin_fragments* f, void* hip_stream, char* err, size_t errlen) {
    if (!b || !f) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int crc = check_even_fragments(b->n_reads, err, errlen)) return crc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (const int orc = acc_add_open(b, f, st, err, errlen)) return orc;
    const int rc = fin_launch_fragments(b->last_frec ? b->d_frec : nullptr, (const uint64_t*)b->d_out_offs, b->d_out, (uint32_t)(b->n_reads / 2), b->dev.k, f->d_ends,
                                        (uint32_t)f->n_unitigs, f->n_bins, f->bin_width, nullptr, f->d_buf, fragments_counters(f), fragments_flags(f), b->d_ovf_count,
                                        b->last_ovf_cap, st);
    return acc_add_close(f, st, rc, "fragments kernel: ", err, errlen);
}

int fin_fragments_download(fin_fragments* f, uint64_t* hist_out, uint64_t counters_out[7], char* err, size_t errlen) {
    if (!f) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int orc = acc_download_open(f, fragments_flags(f), PILEUP_WITHHELD, PILEUP_OUTSIDE, err, errlen)) return orc;
    if (hist_out) HIPCHK(hipMemcpy(hist_out, f->d_buf, (size_t)f->n_bins * 8, hipMemcpyDeviceToHost));
    if (counters_out) HIPCHK(hipMemcpy(counters_out, fragments_counters(f), 56, hipMemcpyDeviceToHost));
    return FIN_OK;
}

// the batch's own fragments: fin_fragment[n_reads / 2] and, behind them, the flag word the kernel wants (nobody reads it: an outside mate is not placed)
int fin_batch_fragments(fin_batch* b, uint64_t* n_frags, char* err, size_t errlen) {
    if (!b) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (n_frags) *n_frags = 0;
    if (!b->ran) { set_err(err, errlen, "this batch has not run: there are no fragments to make (fin_batch_run first)"); return FIN_EINVAL; }
    if (const int crc = check_even_fragments(b->n_reads, err, errlen)) return crc;
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    b->frag_ready = false;
    if (b->n_kmers != 0) if (const int orc = batch_overrun_check(b, st, err, errlen)) return orc;   // a run without results: nothing is written
    const uint32_t nf = (uint32_t)(b->n_reads / 2);
    if (batch_grow(b, &b->d_frag, b->cap_frag, (size_t)nf * 16 + 16, st)) { set_err(err, errlen, "out of device memory (fragments)"); return FIN_ENOMEM; }
    uint32_t* const d_flags = (uint32_t*)((uint8_t*)b->d_frag + (size_t)nf * 16);
    HIPCHK(hipMemsetAsync(d_flags, 0, 16, st));
    const int rc = fin_launch_fragments(b->n_kmers != 0 && b->last_frec ? b->d_frec : nullptr, (const uint64_t*)b->d_out_offs, b->d_out, nf, b->dev.k, b->dev.ends,
                                        (uint32_t)b->idx->n_unitigs, 0, 0, b->d_frag, nullptr, nullptr, d_flags, nullptr, 0, st);
    if (rc != 0) { set_err(err, errlen, std::string("fragments kernel: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
    b->frag_ready = true;
    if (n_frags) *n_frags = nf;
    return FIN_OK;
}

void* fin_batch_device_fragments(const fin_batch* b) { return b && b->frag_ready ? b->d_frag : nullptr; }

int fin_batch_download_fragments(fin_batch* b, fin_fragment* out, char* err, size_t errlen) {
    if (!b) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (!b->frag_ready) { set_err(err, errlen, "fin_batch_fragments first"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = b->last_stream;
    const size_t nf = (size_t)(b->n_reads / 2);
    if (nf && out) HIPCHK(hipMemcpyAsync(out, b->d_frag, nf * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FIN_OK;
}

// ---- links: the junctions reads cross (fin_links.hip) --------------------------------------------------------------------------------------
struct fin_links : fin_acc {
    uint64_t n_unitigs = 0, total_len = 0, max_links = 0;
    uint32_t cap = 0;                     // slots: a power of two, 4 .. 2^29
    const uint32_t* d_ends = nullptr;     // the replica's ends_p
    void* d_tab = nullptr;                // cap slots of {u64 key, u64 count}, then the trailer: u64 n_distinct, the flag word (fin_launch_links_add)
};
static_assert(sizeof(fin_link) == 24, "fin_link is 24 bytes on both sides");
static uint64_t* links_ctr(const fin_links* l) { return (uint64_t*)l->d_tab + 2 * (size_t)l->cap; }
static size_t links_bytes(const fin_links* l) { return (size_t)l->cap * 16 + FIN_LINKS_TRAILER; }

void fin_links_free(fin_links* l) {
    if (!acc_free_open(l)) return;
    (void)hipFree(l->d_tab);
    delete l;
}

int fin_links_create(const fin_index* idx, int device, uint64_t max_links, fin_links** out, char* err, size_t errlen) {
    if (!idx || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    *out = nullptr;
    if (max_links == 0 || max_links > FIN_LINKS_MAX) { set_err(err, errlen, "max_links is 1 .. 2^28"); return FIN_ELIMIT; }
    const fin_index::Replica* rep = nullptr;
    if (const int orc = acc_create_open(idx, device, &rep, err, errlen)) return orc;
    fin_links* l = acc_new<fin_links>(idx, device, err, errlen);
    if (!l) return FIN_ENOMEM;
    l->n_unitigs = idx->n_unitigs; l->total_len = idx->total_len; l->max_links = max_links; l->d_ends = rep->dev.ends;
    l->cap = 4;
    while ((uint64_t)l->cap < 2 * max_links) l->cap <<= 1;
    if (hipMalloc(&l->d_tab, links_bytes(l)) != hipSuccess) { (void)hipGetLastError(); delete l; set_err(err, errlen, "out of device memory (table of links)"); return FIN_ENOMEM; }
    const int rc = fin_launch_links_clear(l->d_tab, l->cap, nullptr);
    if (rc != 0 || hipStreamSynchronize(nullptr) != hipSuccess) { (void)hipGetLastError(); fin_links_free(l); set_err(err, errlen, "links clear kernel failed"); return FIN_ENODEV; }
    *out = l;
    return FIN_OK;
}

// the empty key is all ones, so the reset is a small kernel, not a memset: ordered as a reset is (AccPending::reform)
int fin_links_reset(fin_links* l, void* hip_stream) {
    if (!l) return FIN_EINVAL;
    if (hipSetDevice(l->device) != hipSuccess) return FIN_ENODEV;
    hipStream_t st = (hipStream_t)hip_stream;
    return l->pend.reform(st, [&]() -> int { return fin_launch_links_clear(l->d_tab, l->cap, st) == 0 ? FIN_OK : FIN_ENODEV; }, nullptr, 0);
}

void* fin_links_device_table(const fin_links* l) { return l ? l->d_tab : nullptr; }
uint64_t fin_links_capacity(const fin_links* l) { return l ? l->cap : 0; }

int fin_batch_add_links(fin_batch* b, fin_links* l, void* hip_stream, char* err, size_t errlen) {
    if (!b || !l) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    hipStream_t st = (hipStream_t)hip_stream;
    if (const int orc = acc_add_open(b, l, st, err, errlen)) return orc;
    int rc = 0;
    if (l->n_unitigs != 0 && l->total_len != 0 && b->n_kmers != 0)
        rc = fin_launch_links_add(b->last_frec ? b->d_frec : nullptr, (const uint64_t*)b->d_out_offs, b->d_out, (uint32_t)b->n_reads, l->d_ends, (uint32_t)l->n_unitigs,
                                  l->total_len, l->d_tab, l->cap, l->max_links, b->d_ovf_count, b->last_ovf_cap, st);
    return acc_add_close(l, st, rc, "links kernel: ", err, errlen);
}

int fin_links_download(fin_links* l, uint64_t min_count, fin_link* links_out, uint64_t cap_out, uint64_t* n_links, uint64_t counters_out[4], char* err, size_t errlen) {
    if (!l || !n_links) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    *n_links = 0;
    if (const int orc = acc_download_open(l, nullptr, nullptr, nullptr, err, errlen)) return orc;
    uint64_t trailer[2] = {0, 0};   // n_distinct, the flag word
    HIPCHK(hipMemcpy(trailer, links_ctr(l), sizeof trailer, hipMemcpyDeviceToHost));
    const uint32_t flags = (uint32_t)trailer[1];
    if (flags & 1u) { set_err(err, errlen, PILEUP_WITHHELD); return FIN_ELIMIT; }
    if (flags & 2u) { set_err(err, errlen, "a transition with a unitig number or a place outside the index was met (not counted; reset the accumulator)"); return FIN_EINVAL; }
    if ((flags & 4u) || trailer[0] > l->max_links) { set_err(err, errlen, "more than max_links distinct links (max_links = " + std::to_string(l->max_links) + "; reset the accumulator)"); return FIN_ELIMIT; }
    if (min_count == 0) min_count = 1;
    // compaction on the device: the slots to keep counted per block, scanned, written as fin_link into a dense list -- the table itself never crosses PCIe
    const uint32_t nb = fin_links_blocks(l->cap);
    void* d_tmp = nullptr; void* d_dense = nullptr;
    const size_t off_bytes = (size_t)nb * 8 + 24, sum_bytes = (size_t)nb * 4;   // blk_off | total | stats[2] | blk_sum
    if (hipMalloc(&d_tmp, off_bytes + sum_bytes) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "out of device memory (compaction of the links)"); return FIN_ENOMEM; }
    uint64_t* const d_off = (uint64_t*)d_tmp; uint64_t* const d_total = d_off + nb; uint32_t* const d_sum = (uint32_t*)((char*)d_tmp + off_bytes);
    hipError_t he = hipMemsetAsync(d_total, 0, 24, nullptr);
    if (he == hipSuccess) he = (hipError_t)fin_launch_links_count(l->d_tab, l->cap, min_count, d_sum, d_off, d_total, d_total + 1, nullptr);
    uint64_t res[3] = {0, 0, 0};   // kept, the sum of the counts, self links
    if (he == hipSuccess) he = hipMemcpy(res, d_total, sizeof res, hipMemcpyDeviceToHost);
    const uint64_t total = res[0];
    std::vector<fin_link> links;
    if (he == hipSuccess && links_out && total && total <= cap_out && l->n_unitigs) {
        links.resize((size_t)total);
        he = hipMalloc(&d_dense, (size_t)total * sizeof(fin_link));
        if (he == hipSuccess) he = (hipError_t)fin_launch_links_write(l->d_tab, l->cap, min_count, d_off, l->d_ends, (uint32_t)l->n_unitigs, d_dense, nullptr);
        if (he == hipSuccess) he = hipMemcpy(links.data(), d_dense, (size_t)total * sizeof(fin_link), hipMemcpyDeviceToHost);
    }
    (void)hipFree(d_tmp); (void)hipFree(d_dense);
    if (he != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, std::string("compaction of the links: ") + hipGetErrorString(he)); return FIN_ENODEV; }
    *n_links = total;
    if (counters_out) { counters_out[0] = res[1]; counters_out[1] = trailer[0]; counters_out[2] = total; counters_out[3] = res[2]; }
    if (!links_out) return FIN_OK;
    if (total > cap_out) { set_err(err, errlen, "room for " + std::to_string(cap_out) + " links, " + std::to_string(total) + " needed"); return FIN_ELIMIT; }
    // the canonical order, ascending by (g_a, g_b): places ascend with (u, off)
    std::sort(links.begin(), links.end(), [](const fin_link& x, const fin_link& y) {
        return std::make_tuple(x.u_a, x.off_a, x.u_b, x.off_b) < std::make_tuple(y.u_a, y.off_a, y.u_b, y.off_b);
    });
    if (total) memcpy(links_out, links.data(), (size_t)total * sizeof(fin_link));
    return FIN_OK;
}

int fin_batch_step_time(const fin_batch* b, uint64_t skip_first, double ms_parts[5], uint64_t* n_runs) {
    if (!b) return FIN_EINVAL;
    double t[5] = {0, 0, 0, 0, 0}; uint64_t n = 0;
    (void)hipSetDevice(b->device);
    for (size_t i = (size_t)skip_first; i < b->runs.size(); i++) {
        const fin_batch::RunEvents& r = b->runs[i];
        if (hipEventSynchronize(r.e[4]) != hipSuccess) continue;
        float tot = 0;
        if (hipEventElapsedTime(&tot, r.e[0], r.e[4]) != hipSuccess) { (void)hipGetLastError(); continue; }
        // events a kernel variant does not record (no pre-pass, empty batch) fold their interval into the next recorded one
        float part[4] = {0, 0, 0, 0};
        int prev = 0;
        for (int j = 1; j <= 4; j++) {
            if (hipEventQuery(r.e[j]) != hipSuccess) { (void)hipGetLastError(); continue; }
            float d = 0;
            if (hipEventElapsedTime(&d, r.e[prev], r.e[j]) != hipSuccess) { (void)hipGetLastError(); continue; }
            part[j - 1] = d; prev = j;
        }
        for (int j = 0; j < 4; j++) t[j] += part[j];
        t[4] += tot; n++;
    }
    if (ms_parts) for (int j = 0; j < 5; j++) ms_parts[j] = n ? t[j] / (double)n : 0.0;
    if (n_runs) *n_runs = n;
    return FIN_OK;
}

int fin_batch_kernel_time(const fin_batch* b, double* ms_avg, uint64_t* n_runs) {
    double p[5];
    const int rc = fin_batch_step_time(b, 0, p, n_runs);
    if (rc == FIN_OK && ms_avg) *ms_avg = p[4];
    return rc;
}

extern "C" void fin_debug_dump_w(void);
extern "C" void fin_debug_dump_pp(void);
void fin_debug_time(void) { fin_debug_dump_time(); fin_debug_dump_w(); fin_debug_dump_pp(); }

int fin_batch_pipeline_counts(fin_batch* b, uint32_t* out, uint32_t n_words) {
    if (!b || !out) return FIN_EINVAL;
    for (uint32_t i = 0; i < n_words; i++) out[i] = 0;
    if (!b->d_ctr || !b->ran) return FIN_OK;
    if (hipSetDevice(b->device) != hipSuccess || hipStreamSynchronize(b->last_stream) != hipSuccess) return FIN_ENODEV;
    const uint32_t n = std::min<uint32_t>(n_words, fin_v4_counter_words());
    return hipMemcpy(out, b->d_ctr, n * 4, hipMemcpyDeviceToHost) == hipSuccess ? FIN_OK : FIN_ENODEV;
}

// what the most recent fin_batch_run decided (the per-run decision, not a guess from the replica): out[0] the kernel that ran
// (after the k > 128 rule), [1] 1 = nothing prefilled the output (the pipeline wrote every slot once), [2] 1 = second strands were deferred,
// [3] 1 = the pre-pass's fast path was on
// diagnostic (tests of the fused ingest): the most recent run's packed chunks (n_chunks of 16 bytes, may be NULL) and pre-pass verdicts
// (2 * n_reads words, may be NULL); *fused = 1 when that run's ingest was the fast pre-pass's.  Synchronises the run's stream.
int fin_batch_debug_ingest(const fin_batch* b, uint32_t* fused, void* chunks, uint64_t n_chunks, uint32_t* pass, uint64_t n_pass_words) {
    if (!b || !fused) return FIN_EINVAL;
    *fused = b->ran && b->last_fused ? 1u : 0u;
    if (!b->ran) return FIN_OK;
    if (n_chunks > b->n_chunks || n_pass_words > 2 * b->n_reads) return FIN_EINVAL;
    if (hipSetDevice(b->device) != hipSuccess || hipStreamSynchronize(b->last_stream) != hipSuccess) return FIN_ENODEV;
    if (chunks && n_chunks && hipMemcpy(chunks, b->d_packed, n_chunks * 16, hipMemcpyDeviceToHost) != hipSuccess) return FIN_ENODEV;
    if (pass && n_pass_words && hipMemcpy(pass, b->d_pass, n_pass_words * 4, hipMemcpyDeviceToHost) != hipSuccess) return FIN_ENODEV;
    return FIN_OK;
}

int fin_batch_run_info(const fin_batch* b, uint32_t out[4]) {
    if (!b || !out) return FIN_EINVAL;
    out[0] = b->last_kernel; out[1] = b->last_no_prefill; out[2] = b->ran ? b->dev.defer_ok : 0u; out[3] = (b->ran && b->dev.defer_ok && b->last_no_prefill) ? b->dev.fast_path : 0u;
    return FIN_OK;
}

int64_t fin_batch_overflow_reads(fin_batch* b) {
    if (!b) return -1;
    if (!b->ran) return 0;
    if (hipSetDevice(b->device) != hipSuccess || hipStreamSynchronize(b->last_stream) != hipSuccess) return -1;
    uint32_t c = 0;
    if (hipMemcpy(&c, b->d_ovf_count, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)c;   // (entries of the list: under kernel 4 a read may be on it more than once)
}

// reads [lo, hi) of a flat read set on one device; pairs_out points at read lo's first pair.
// The range is cut into sub-batches that a few host threads push through reusable device batches, each on its own stream:
// while one sub-batch is being searched, the previous one's pairs travel back over PCIe and the next one's reads travel in
// (H2D + kernel + D2H double-buffered).  With page-locked caller buffers (fin_host_alloc) the copies are DMA at
// link speed; pageable buffers work too, staged by the runtime.
// What an entry point does with one searched sub-batch is its PRODUCT: `take` runs on the worker's thread behind fin_batch_run (text mode 2: the pairs are not the
// product) with the batch, the sub-batch's place in the caller's read set and `pos`, to which it adds what the entry point reports as found; a code other than
// FIN_OK and a message in `e` end the search.  Products whose sub-batches land one behind the other in a caller buffer (text, records, segments) name their
// Landing: the pipeline sizes it and gives it up when a worker fails.  Without a product the pairs themselves come back (fin_search_batch, _multi)
struct SubBatch { size_t i; uint64_t lo, hi, pair_off; };   // reads [lo, hi) of the caller's set; pair_off: the k-mers of the range's reads before lo
struct Product {
    uint64_t group = 1;   // reads that a sub-batch boundary never separates (2: interleaved mates)
    Landing* landing = nullptr;
    std::function<int(fin_batch*, const SubBatch&, uint64_t& pos, char* e, size_t elen)> take;
};

static int search_range_on(const fin_index* idx, int device, const char* bases, const uint64_t* offsets, uint64_t lo, uint64_t hi,
                           int strands, int32_t* pairs_out, uint64_t* n_positive, char* err, size_t errlen, const Product* product = nullptr) {
    // A device batch addresses k-mers and bases with 32 bits (also bounds the HBM one sub-batch takes)
    const uint64_t MAX_BASES = 1ull << 31, MAX_READS = 1ull << 26;
    const uint64_t MAX_KMERS = std::min<uint64_t>((uint64_t)optv(idx, O_max_batch_kmers), (uint64_t)optv(idx, O_pipeline_kmers));
    const uint64_t k = idx->k, group = product ? product->group : 1;
    std::vector<SubBatch> subs;
    {
        uint64_t pair_off = 0;
        do {
            uint64_t h2 = lo, nb = 0, nk = 0;
            while (h2 < hi) {   // a group of `group` reads at a time (1, or 2: a pair of mates is never split); the first group is always taken
                const uint64_t g2 = std::min<uint64_t>(h2 + group, hi);
                uint64_t glen = 0, gkk = 0;
                for (uint64_t r = h2; r < g2; r++) {
                    const uint64_t len = offsets[r + 1] - offsets[r];
                    glen += len; gkk += len >= k ? len - k + 1 : 0;
                }
                if (h2 > lo && (nb + glen > MAX_BASES || nk + gkk > MAX_KMERS || g2 - lo > MAX_READS)) break;
                nb += glen; nk += gkk; h2 = g2;
            }
            subs.push_back(SubBatch{subs.size(), lo, h2, pair_off});
            pair_off += nk; lo = h2;
        } while (lo < hi);
    }
    Landing* const landing = product ? product->landing : nullptr;
    if (landing) landing->reset(subs.size());
    const uint64_t hi_bases = offsets[subs.back().hi] - offsets[subs.front().lo];
    const int n_workers = (int)std::min<size_t>(subs.size(), (size_t)optv(idx, O_pipeline_depth));
    std::atomic<size_t> next{0};
    std::atomic<int> first_rc{FIN_OK};
    std::atomic<uint64_t> pos_total{0};
    std::mutex err_mu;
    const bool stage_in = optv(idx, O_stage_pageable) && hi_bases > 0 && !is_page_locked(bases + offsets[subs[0].lo]);
    const bool stage_out = optv(idx, O_stage_pageable) && pairs_out && !is_page_locked(pairs_out);
    auto worker = [&]() {
        fin_batch* b = nullptr;
        char e[512] = {0};
        void* sin = nullptr; size_t sin_cap = 0; void* sout = nullptr; size_t sout_cap = 0;
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= subs.size() || first_rc.load() != FIN_OK) break;
            const SubBatch& s = subs[i];
            int rc = FIN_OK;
            const char* first = bases ? bases + offsets[s.lo] : nullptr;
            const size_t nb = (size_t)(offsets[s.hi] - offsets[s.lo]);
            if (stage_in && nb) {
                if (nb > sin_cap) { g_stage.put(sin, sin_cap); sin = g_stage.get(nb, &sin_cap); }
                if (!sin) { rc = FIN_ENOMEM; snprintf(e, sizeof e, "page-locked staging buffer: out of memory"); }
                else { memcpy(sin, first, nb); first = (const char*)sin; }
            }
            if (rc == FIN_OK) {
                if (!b) {   // a batch the pipeline used before on this device, if there is one
                    std::lock_guard<std::mutex> g(idx->pool_mu);
                    for (size_t j = 0; j < idx->batch_pool.size(); j++)
                        if (idx->batch_pool[j].first == device) { b = idx->batch_pool[j].second; idx->batch_pool.erase(idx->batch_pool.begin() + (long)j); break; }
                }
                if (!b) {
                    const fin_index::Replica* rep = idx->replica_on(device);
                    b = new (std::nothrow) fin_batch();
                    if (!b || !rep) { rc = FIN_ENOMEM; snprintf(e, sizeof e, "out of memory"); }
                    else { b->idx = idx; b->dev = rep->dev; b->device = device; }
                }
                if (rc == FIN_OK) rc = batch_load(b, first, offsets + s.lo, s.hi - s.lo, e, sizeof e);
            }
            if (rc == FIN_OK) { b->text_mode = product ? 2 : 0; rc = fin_batch_run(b, strands, (void*)b->own_stream, e, sizeof e); }   // (a product: the pairs are not kept for the host)
            uint64_t pos = 0;
            if (rc == FIN_OK && product) rc = product->take(b, s, pos, e, sizeof e);
            else
            if (rc == FIN_OK) {
                int32_t* dst = pairs_out ? pairs_out + 2 * s.pair_off : nullptr;
                const size_t ob = (size_t)b->n_kmers * 8;
                if (stage_out && ob) {
                    if (ob > sout_cap) { g_stage.put(sout, sout_cap); sout = g_stage.get(ob, &sout_cap); }
                    if (!sout) { rc = FIN_ENOMEM; snprintf(e, sizeof e, "page-locked staging buffer: out of memory"); }
                    else {
                        rc = fin_batch_download(b, (int32_t*)sout, n_positive ? &pos : nullptr, e, sizeof e);
                        if (rc == FIN_OK) memcpy(dst, sout, ob);
                    }
                } else rc = fin_batch_download(b, dst, n_positive ? &pos : nullptr, e, sizeof e);
            }
            if (rc != FIN_OK) {
                int expect = FIN_OK;
                if (first_rc.compare_exchange_strong(expect, rc)) { std::lock_guard<std::mutex> g(err_mu); set_err(err, errlen, e); }
                if (landing) landing->give_up();   // nobody may wait for the sub-batches this worker will not do
                break;
            }
            pos_total += pos;
        }
        if (b && first_rc.load() == FIN_OK) {   // kept for the next call (at most 8 per index)
            std::lock_guard<std::mutex> g(idx->pool_mu);
            if (idx->batch_pool.size() < 8) { idx->batch_pool.push_back({device, b}); b = nullptr; }
        }
        fin_batch_free(b);
        g_stage.put(sin, sin_cap); g_stage.put(sout, sout_cap);
    };
    if (n_workers <= 1) worker();
    else {
        std::vector<std::thread> th;
        for (int w = 0; w < n_workers; w++) th.emplace_back(worker);
        for (auto& t : th) t.join();
    }
    if (first_rc.load() != FIN_OK) return first_rc.load();
    if (n_positive) *n_positive = pos_total.load();
    return FIN_OK;
}

// the opening that the fin_search_batch_* entry points share, behind their argument test: where the search runs.  With `beside` (a labelling, a colour matrix, an
// accumulator) that is its device, and it must belong to the index -- else `other_index` is the message; without, the index's first replica, and there must be one
static int search_home(const fin_index* idx, const fin_acc* beside, const char* other_index, int* device, char* err, size_t errlen) {
    if (beside) {
        if (beside->idx != idx) { set_err(err, errlen, other_index); return FIN_EINVAL; }
        *device = beside->device;
        return FIN_OK;
    }
    if (idx->replicas.empty()) { set_err(err, errlen, "index is not resident on a device: call fin_index_to_device first (no CPU fallback)"); return FIN_ENODEV; }
    *device = idx->replicas[0].device;
    return FIN_OK;
}
// ... and with the argument test of all but the three oldest: `rest_ok` is what the entry point asks of its own pointers (`beside` not null among it)
static int search_open(const fin_index* idx, const uint64_t* offsets, int strands, bool rest_ok, const fin_acc* beside, const char* other_index, int* device, char* err,
                       size_t errlen) {
    if (!idx || !offsets || !rest_ok || (strands != FIN_FWD && strands != FIN_MERGED)) { set_err(err, errlen, "bad argument"); return FIN_EINVAL; }
    return search_home(idx, beside, other_index, device, err, errlen);
}
static const char* const OTHER_LABELS = "the labelling belongs to another index";
static const char* const OTHER_COLORS = "the colours belong to another index";
static const char* const OTHER_EQCLASSES = "the equivalence classes belong to another index";
static const char* const OTHER_ACC = "the accumulator belongs to another index";

// ---- the streaming loop with the reference's text as its result (search_fmin.hh:43-72 including :62-65) ----
struct fin_text { void* p = nullptr; size_t cap = 0; uint64_t size = 0; };
fin_text* fin_text_create(void) { return new (std::nothrow) fin_text(); }
void fin_text_free(fin_text* t) { if (t) { if (t->p) (void)hipHostFree(t->p); delete t; } }
int fin_text_reserve(fin_text* t, uint64_t bytes) {   // page-lock room ahead of time (about 0.15 s per GB: worth doing beside other start-up work)
    if (!t) return FIN_EINVAL;
    if (bytes <= t->cap) return FIN_OK;
    if (t->p) (void)hipHostFree(t->p);
    t->p = nullptr; t->cap = 0; t->size = 0;
    if (hipHostMalloc(&t->p, bytes, hipHostMallocDefault) != hipSuccess) return FIN_ENOMEM;
    t->cap = bytes;
    return FIN_OK;
}
const char* fin_text_data(const fin_text* t) { return t ? (const char*)t->p : nullptr; }
uint64_t fin_text_size(const fin_text* t) { return t ? t->size : 0; }

// the whole read set through the pipeline with a product, on `device`
static int search_product(const fin_index* idx, int device, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, const Product& p,
                          uint64_t* n_positive, char* err, size_t errlen) {
    return search_range_on(idx, device, bases, offsets, 0, n_reads, strands, nullptr, n_positive, err, errlen, &p);
}
// (an add goes behind the run on the batch's own stream: the next batch_load on that stream finds it done; the accumulator's download waits for the last ones)
static void* own(const fin_batch* b) { return (void*)b->own_stream; }

int fin_search_batch_text(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, fin_text* out,
                          uint64_t* n_positive, char* err, size_t errlen) {
    if (!idx || !offsets || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    int device = -1;
    if (const int orc = search_home(idx, nullptr, nullptr, &device, err, errlen)) return orc;
    if (n_positive) *n_positive = 0;
    out->size = 0;
    if (n_reads == 0) return FIN_OK;
    const uint64_t k = idx->k;
    uint64_t nk = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        const uint64_t len = offsets[r + 1] - offsets[r];
        if (len < k) { set_err(err, errlen, "a read without k-mers: its empty line belongs to no pair (format such batches on the host)"); return FIN_EINVAL; }
        nk += len - k + 1;
    }
    // no pair's text is longer than "(last unitig,last offset of the longest unitig)" + separator, nor shorter than "(-1,-1) "
    uint64_t max_len = 1;
    for (uint64_t u = 0; u < idx->n_unitigs; u++) max_len = std::max<uint64_t>(max_len, (uint64_t)idx->ends[u + 1] - idx->ends[u]);
    auto ndig = [](uint64_t v) { uint64_t n = 1; while (v >= 10) { v /= 10; n++; } return n; };
    const uint64_t per_pair = std::max<uint64_t>(8, 4 + ndig(idx->n_unitigs ? idx->n_unitigs - 1 : 0) + ndig(max_len - 1));
    const uint64_t need = per_pair * nk + 64;
    if (need > out->cap) {
        if (out->p) (void)hipHostFree(out->p);
        out->p = nullptr; out->cap = 0;
        if (hipHostMalloc(&out->p, need + need / 16, hipHostMallocDefault) != hipSuccess) { set_err(err, errlen, "page-locked text buffer: out of memory"); return FIN_ENOMEM; }
        out->cap = need + need / 16;
    }
    // the text is made on the device; its place in the caller's buffer is behind the text of all earlier sub-batches
    Landing land;
    Product p; p.landing = &land;
    p.take = [&](fin_batch* b, const SubBatch& s, uint64_t& pos, char* e, size_t elen) -> int {
        uint64_t L = 0;
        if (const int rc = fin_batch_format_text(b, &L, e, elen)) return rc;
        const uint64_t at = land.place(s.i, L);
        if (at + L > out->cap) { snprintf(e, elen, "text buffer too small"); return FIN_ELIMIT; }
        if (const int rc = fin_batch_download_text(b, (char*)out->p + at, e, elen)) return rc;
        return n_positive ? fin_batch_download(b, nullptr, &pos, e, elen) : FIN_OK;
    };
    const int rc = search_product(idx, device, bases, offsets, n_reads, strands, p, n_positive, err, errlen);
    if (rc == FIN_OK) out->size = land.total();
    return rc;
}

int fin_search_batch_records(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, fin_read_record* recs_out,
                             int32_t* stream_pairs_out, uint64_t stream_cap_pairs, uint64_t* n_stream_pairs, char* err, size_t errlen) {
    if (!idx || !offsets || (n_reads && !recs_out)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    int device = -1;
    if (const int orc = search_home(idx, nullptr, nullptr, &device, err, errlen)) return orc;
    if (n_stream_pairs) *n_stream_pairs = 0;
    if (n_reads == 0) return FIN_OK;
    // the sub-batch's stream of pairs lands behind the streams of all earlier sub-batches, its records at its reads' numbers
    const uint64_t cap = stream_pairs_out ? stream_cap_pairs : 0;
    Landing land;
    Product p; p.landing = &land;
    p.take = [&](fin_batch* b, const SubBatch& s, uint64_t&, char* e, size_t elen) -> int {
        uint64_t L = 0;
        if (const int rc = fin_batch_records(b, &L, e, elen)) return rc;
        const uint64_t at = land.place(s.i, L);
        if (at + L > cap) { snprintf(e, elen, "pair stream buffer too small"); return FIN_ELIMIT; }
        return fin_batch_download_records(b, recs_out + s.lo, stream_pairs_out ? stream_pairs_out + 2 * at : nullptr, e, elen);
    };
    const int rc = search_product(idx, device, bases, offsets, n_reads, FIN_MERGED, p, nullptr, err, errlen);
    if (rc == FIN_OK && n_stream_pairs) *n_stream_pairs = land.total();
    return rc;
}

int fin_search_batch_segments(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, uint64_t* seg_offs_out,
                              fin_segment* segs_out, uint64_t seg_cap, uint64_t* n_segments, uint64_t* n_positive, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, seg_offs_out && (!seg_cap || segs_out), nullptr, nullptr, &device, err, errlen)) return orc;
    if (n_segments) *n_segments = 0;
    if (n_positive) *n_positive = 0;
    seg_offs_out[0] = 0;
    if (n_reads == 0) return FIN_OK;
    // made behind the run on the device; the sub-batch's segments land behind those of all earlier sub-batches, its seg_offs at its reads' numbers, rebased to the
    // whole read set.  Once they no longer fit nothing more is copied; the sub-batches go on being counted, so the caller learns how many there are
    const uint64_t cap = segs_out ? seg_cap : 0;
    std::atomic<bool> over{false};
    Landing land;
    Product p; p.landing = &land;
    p.take = [&](fin_batch* b, const SubBatch& s, uint64_t& pos, char* e, size_t elen) -> int {
        uint64_t L = 0;
        if (const int rc = fin_batch_segments(b, &L, e, elen)) return rc;
        const uint64_t at = land.place(s.i, L);
        if (at + L > cap) { over.store(true); return FIN_OK; }
        if (over.load()) return FIN_OK;
        std::vector<uint64_t> so((size_t)(s.hi - s.lo) + 1);
        if (const int rc = fin_batch_download_segments(b, so.data(), segs_out ? segs_out + at : nullptr, e, elen)) return rc;
        uint64_t* const dst = seg_offs_out + s.lo;   // (entry 0 is the sub-batch before's last, or the caller's)
        for (size_t r = 1; r < so.size(); r++) dst[r] = so[r] + at;
        for (uint64_t q = 0; q < L; q++) { const int32_t n = segs_out[at + q].len; pos += (uint64_t)(n < 0 ? -(int64_t)n : (int64_t)n); }
        return FIN_OK;
    };
    uint64_t pos = 0;
    const int rc = search_product(idx, device, bases, offsets, n_reads, strands, p, &pos, err, errlen);
    if (rc != FIN_OK) return rc;
    const uint64_t total = land.total();
    if (n_segments) *n_segments = total;
    if (over.load()) {
        set_err(err, errlen, "segment buffer too small: room for " + std::to_string(cap) + " segments, " + std::to_string(total) + " needed");
        return FIN_ELIMIT;
    }
    if (n_positive) *n_positive = pos;
    return FIN_OK;
}

int fin_search_batch_read_summaries(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, fin_read_summary* out,
                                    uint64_t* n_positive, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, !n_reads || out, nullptr, nullptr, &device, err, errlen)) return orc;
    if (n_positive) *n_positive = 0;
    if (n_reads == 0) return FIN_OK;
    Product p;   // a sub-batch's summaries land at its reads' numbers
    p.take = [&](fin_batch* b, const SubBatch& s, uint64_t& pos, char* e, size_t elen) -> int {
        if (const int rc = fin_batch_read_summaries(b, e, elen)) return rc;
        fin_read_summary* const dst = out + s.lo;
        if (const int rc = fin_batch_download_read_summaries(b, dst, e, elen)) return rc;
        for (uint64_t r = 0; r < s.hi - s.lo; r++) pos += dst[r].n_found;
        return FIN_OK;
    };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, n_positive, err, errlen);
}

int fin_search_batch_screen(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, uint32_t min_found, uint32_t min_permille,
                            int invert, uint64_t* bits_out, uint64_t* n_pass, char* err, size_t errlen) {
    // (not search_open: this entry point tests its threshold before the index's residence, and coinciding faults keep reporting the same one)
    if (!idx || !offsets || (strands != FIN_FWD && strands != FIN_MERGED)) { set_err(err, errlen, "bad argument"); return FIN_EINVAL; }
    if (const int crc = check_permille(min_permille, BAD_MIN_PERMILLE, err, errlen)) return crc;
    int device = -1;
    if (const int orc = search_home(idx, nullptr, nullptr, &device, err, errlen)) return orc;
    if (n_pass) *n_pass = 0;
    if (n_reads == 0) return FIN_OK;
    if (bits_out) for (uint64_t w = 0; w < (n_reads + 63) / 64; w++) bits_out[w] = 0;
    std::atomic<uint64_t> pass{0};
    std::mutex bits_mu;   // (neighbouring sub-batches share a word)
    Product p;
    p.take = [&](fin_batch* b, const SubBatch& s, uint64_t&, char* e, size_t elen) -> int {
        uint64_t np = 0;
        if (const int rc = fin_batch_screen(b, min_found, min_permille, invert, &np, e, elen)) return rc;
        pass += np;
        if (!bits_out) return FIN_OK;
        // the sub-batch's bitmap begins at bit 0; in the whole read set's it begins at its first read's bit, which need not start a word
        const uint64_t n = s.hi - s.lo, at = s.lo;
        std::vector<uint64_t> w((size_t)((n + 63) / 64) + 1, 0);
        if (const int rc = fin_batch_download_screen(b, nullptr, w.data(), e, elen)) return rc;
        const uint32_t sh = (uint32_t)(at & 63);
        std::lock_guard<std::mutex> g(bits_mu);
        for (size_t q = 0; q + 1 < w.size(); q++) {
            if (!w[q]) continue;
            bits_out[(at >> 6) + q] |= w[q] << sh;
            if (sh && (w[q] >> (64u - sh))) bits_out[(at >> 6) + q + 1] |= w[q] >> (64u - sh);   // (a set bit is a read below s.hi: the word exists)
        }
        return FIN_OK;
    };
    const int rc = search_product(idx, device, bases, offsets, n_reads, strands, p, nullptr, err, errlen);
    if (rc == FIN_OK && n_pass) *n_pass = pass.load();
    return rc;
}

int fin_search_batch_classify(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, const fin_labels* l,
                              fin_read_class* out, uint64_t* n_positive, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, l && (!n_reads || out), l, OTHER_LABELS, &device, err, errlen)) return orc;
    if (n_positive) *n_positive = 0;
    if (n_reads == 0) return FIN_OK;
    Product p;   // a sub-batch's classes land at its reads' numbers
    p.take = [&](fin_batch* b, const SubBatch& s, uint64_t& pos, char* e, size_t elen) -> int {
        if (const int rc = fin_batch_classify(b, l, e, elen)) return rc;
        fin_read_class* const dst = out + s.lo;
        if (const int rc = fin_batch_download_read_classes(b, dst, e, elen)) return rc;
        for (uint64_t r = 0; r < s.hi - s.lo; r++) pos += dst[r].n_labelled;
        return FIN_OK;
    };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, n_positive, err, errlen);
}

int fin_search_batch_add_colors(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, fin_colors* c, uint32_t color, char* err,
                                size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, c, c, OTHER_COLORS, &device, err, errlen)) return orc;
    if (color >= c->n_colors) { set_err(err, errlen, "colour " + std::to_string(color) + " is not below n_colors = " + std::to_string(c->n_colors)); return FIN_EINVAL; }
    if (const int drc = colors_want_dense(c, err, errlen)) return drc;
    if (n_reads == 0) return FIN_OK;
    Product p;   // every sub-batch's unitigs get the colour on the device, nothing comes back
    p.take = [&](fin_batch* b, const SubBatch&, uint64_t&, char* e, size_t elen) -> int { return fin_batch_add_colors(b, c, color, own(b), e, elen); };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, nullptr, err, errlen);
}

int fin_search_batch_pseudoalign(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, const fin_colors* c, uint32_t permille,
                                 uint64_t* rows_out, fin_read_pseudo* heads_out, uint64_t* n_positive, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, c && (!n_reads || heads_out), c, OTHER_COLORS, &device, err, errlen)) return orc;
    if (const int crc = check_permille(permille, BAD_PERMILLE, err, errlen)) return crc;
    if (n_positive) *n_positive = 0;
    if (n_reads == 0) return FIN_OK;
    Product p;   // a sub-batch's rows (may be null) and heads land at its reads' numbers
    p.take = [&](fin_batch* b, const SubBatch& s, uint64_t& pos, char* e, size_t elen) -> int {
        if (const int rc = fin_batch_pseudoalign(b, c, permille, e, elen)) return rc;
        fin_read_pseudo* const dst = heads_out + s.lo;
        if (const int rc = fin_batch_download_pseudo(b, rows_out ? rows_out + s.lo * c->words : nullptr, dst, e, elen)) return rc;
        for (uint64_t r = 0; r < s.hi - s.lo; r++) pos += dst[r].n_colored;
        return FIN_OK;
    };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, n_positive, err, errlen);
}

int fin_search_batch_pseudoalign_paired(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, const fin_colors* c,
                                        uint32_t permille, uint32_t mode, uint64_t* rows_out, fin_pair_pseudo* heads_out, uint64_t* n_positive, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, c && (n_reads < 2 || heads_out), c, OTHER_COLORS, &device, err, errlen)) return orc;
    if (const int crc = check_permille(permille, BAD_PERMILLE, err, errlen)) return crc;
    if (const int crc = check_pair_mode(mode, err, errlen)) return crc;
    if (const int crc = check_even(n_reads, err, errlen)) return crc;
    if (n_positive) *n_positive = 0;
    if (n_reads == 0) return FIN_OK;
    // the reads are interleaved mates: a sub-batch ends only after an even number of reads, and the fragments' rows and heads land at the fragments' numbers
    Product p; p.group = 2;
    p.take = [&](fin_batch* b, const SubBatch& s, uint64_t& pos, char* e, size_t elen) -> int {
        if (const int rc = fin_batch_pseudoalign_paired(b, c, permille, mode, e, elen)) return rc;
        const uint64_t at = s.lo / 2;   // (every sub-batch begins at an even read)
        fin_pair_pseudo* const dst = heads_out + at;
        if (const int rc = fin_batch_download_pair_pseudo(b, rows_out ? rows_out + at * c->words : nullptr, dst, e, elen)) return rc;
        for (uint64_t f = 0; f < (s.hi - s.lo) / 2; f++) pos += dst[f].n_colored;
        return FIN_OK;
    };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, n_positive, err, errlen);
}

int fin_search_batch_add_classes(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, fin_labels* l, uint32_t min_found,
                                 uint32_t min_permille, uint32_t min_margin, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, l, l, OTHER_LABELS, &device, err, errlen)) return orc;
    if (const int crc = check_permille(min_permille, BAD_MIN_PERMILLE, err, errlen)) return crc;
    if (n_reads == 0) return FIN_OK;
    Product p;   // every sub-batch is added to the labelling's tally on the device, nothing comes back
    p.take = [&](fin_batch* b, const SubBatch&, uint64_t&, char* e, size_t elen) -> int { return fin_batch_add_classes(b, l, min_found, min_permille, min_margin, own(b), e, elen); };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, nullptr, err, errlen);
}

static const char* const OTHER_TAXONOMY = "the taxonomy belongs to another index";
int fin_search_batch_taxa(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, const fin_taxonomy* t, uint32_t min_found,
                          uint32_t confidence_permille, fin_read_taxon* out, uint64_t* n_positive, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, t && (!n_reads || out), t, OTHER_TAXONOMY, &device, err, errlen)) return orc;
    if (const int crc = check_permille(confidence_permille, BAD_CONFIDENCE, err, errlen)) return crc;
    if (n_positive) *n_positive = 0;
    if (n_reads == 0) return FIN_OK;
    Product p;   // a sub-batch's read taxa land at its reads' numbers
    p.take = [&](fin_batch* b, const SubBatch& s, uint64_t& pos, char* e, size_t elen) -> int {
        if (const int rc = fin_batch_taxa(b, t, min_found, confidence_permille, e, elen)) return rc;
        fin_read_taxon* const dst = out + s.lo;
        if (const int rc = fin_batch_download_read_taxa(b, dst, e, elen)) return rc;
        for (uint64_t r = 0; r < s.hi - s.lo; r++) pos += dst[r].n_labelled;
        return FIN_OK;
    };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, n_positive, err, errlen);
}

int fin_search_batch_add_taxa(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, fin_taxonomy* t, uint32_t min_found,
                              uint32_t confidence_permille, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, t, t, OTHER_TAXONOMY, &device, err, errlen)) return orc;
    if (const int crc = check_permille(confidence_permille, BAD_CONFIDENCE, err, errlen)) return crc;
    if (n_reads == 0) return FIN_OK;
    Product p;   // every sub-batch is added to the taxonomy's tally on the device, nothing comes back
    p.take = [&](fin_batch* b, const SubBatch&, uint64_t&, char* e, size_t elen) -> int { return fin_batch_add_taxa(b, t, min_found, confidence_permille, own(b), e, elen); };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, nullptr, err, errlen);
}

int fin_search_batch_add_eqclasses(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, fin_eqclasses* e, uint32_t permille,
                                   char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, e, e, OTHER_EQCLASSES, &device, err, errlen)) return orc;
    if (const int crc = check_permille(permille, BAD_PERMILLE, err, errlen)) return crc;
    if (n_reads == 0) return FIN_OK;
    Product p;   // every sub-batch is pseudoaligned and added on the device, nothing comes back
    p.take = [&](fin_batch* b, const SubBatch&, uint64_t&, char* em, size_t elen) -> int { return fin_batch_add_eqclasses(b, e, permille, own(b), em, elen); };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, nullptr, err, errlen);
}

int fin_search_batch_add_eqclasses_paired(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, fin_eqclasses* e,
                                          uint32_t permille, uint32_t mode, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, e, e, OTHER_EQCLASSES, &device, err, errlen)) return orc;
    if (const int crc = check_permille(permille, BAD_PERMILLE, err, errlen)) return crc;
    if (const int crc = check_pair_mode(mode, err, errlen)) return crc;
    if (const int crc = check_even(n_reads, err, errlen)) return crc;
    if (n_reads == 0) return FIN_OK;
    Product p; p.group = 2;   // (interleaved mates: no sub-batch splits a pair)
    p.take = [&](fin_batch* b, const SubBatch&, uint64_t&, char* em, size_t elen) -> int { return fin_batch_add_eqclasses_paired(b, e, permille, mode, own(b), em, elen); };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, nullptr, err, errlen);
}

int fin_search_batch_assign(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, fin_assign* a, uint32_t permille,
                            uint32_t unit, uint64_t* rows_out, fin_read_assign* heads_out, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, a && (n_reads < (unit ? 2u : 1u) || heads_out), a, OTHER_ACC, &device, err, errlen)) return orc;
    if (const int crc = check_permille(permille, BAD_PERMILLE, err, errlen)) return crc;
    if (const int crc = check_assign_unit(unit, err, errlen)) return crc;
    if (unit) if (const int crc = check_even(n_reads, err, errlen)) return crc;
    if (n_reads == 0) return FIN_OK;
    // every sub-batch is pseudoaligned, assigned and counted on the device; its assigned rows (may be null) and heads land at its reads' or fragments' numbers
    Product p; p.group = unit ? 2 : 1;   // (interleaved mates: no sub-batch splits a pair, every sub-batch begins at an even read)
    p.take = [&](fin_batch* b, const SubBatch& s, uint64_t&, char* e, size_t elen) -> int {
        if (const int rc = fin_batch_assign(b, a, permille, unit, own(b), e, elen)) return rc;
        const uint64_t at = unit ? s.lo / 2 : s.lo;
        return fin_batch_download_assign(b, rows_out ? rows_out + at * a->words : nullptr, heads_out + at, e, elen);
    };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, nullptr, err, errlen);
}

// the index's numbers of the caller's unitigs: each one's first k-mer, searched forward, must come back as (u, 0)
int fin_index_unitig_numbers(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_seqs, uint32_t* out, char* err, size_t errlen) {
    if (!idx || !offsets || (n_seqs && (!bases || !out))) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (idx->replicas.empty()) { set_err(err, errlen, "index is not resident on a device: call fin_index_to_device first (no CPU fallback)"); return FIN_ENODEV; }
    const uint64_t k = idx->k;
    for (uint64_t i = 0; i < n_seqs; i++)
        if (offsets[i + 1] - offsets[i] < k) { set_err(err, errlen, "sequence " + std::to_string(i) + " is shorter than k = " + std::to_string(k) + ": not a unitig of this index"); return FIN_EINVAL; }
    if (n_seqs == 0) return FIN_OK;
    std::string firsts((size_t)(n_seqs * k), 'A');
    std::vector<uint64_t> offs((size_t)n_seqs + 1);
    for (uint64_t i = 0; i < n_seqs; i++) { memcpy(&firsts[(size_t)(i * k)], bases + offsets[i], (size_t)k); offs[(size_t)i] = i * k; }
    offs[(size_t)n_seqs] = n_seqs * k;
    std::vector<int32_t> pairs((size_t)n_seqs * 2);
    const int rc = fin_search_batch(idx, firsts.data(), offs.data(), n_seqs, FIN_FWD, pairs.data(), nullptr, err, errlen);
    if (rc != FIN_OK) return rc;
    for (uint64_t i = 0; i < n_seqs; i++) {
        const int32_t u = pairs[(size_t)(2 * i)], off = pairs[(size_t)(2 * i + 1)];
        if (u < 0) { set_err(err, errlen, "sequence " + std::to_string(i) + ": its first k-mer is not in the index -- not a unitig of this index"); return FIN_EINVAL; }
        if (off != 0) {
            set_err(err, errlen, "sequence " + std::to_string(i) + ": its first k-mer is at offset " + std::to_string(off) + " of unitig " + std::to_string(u) + ", not at the start of a unitig");
            return FIN_EINVAL;
        }
        out[i] = (uint32_t)u;
    }
    return FIN_OK;
}

int fin_search_batch_add_hits(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, fin_hits* h, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, h, h, OTHER_ACC, &device, err, errlen)) return orc;
    if (n_reads == 0) return FIN_OK;
    Product p;   // every sub-batch is added on the device, nothing comes back
    p.take = [&](fin_batch* b, const SubBatch&, uint64_t&, char* e, size_t elen) -> int { return fin_batch_add_hits(b, h, own(b), e, elen); };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, nullptr, err, errlen);
}

int fin_search_batch_unitig_counts(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, uint64_t* counts_out,
                                   uint64_t* n_positive, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, !(idx && idx->n_unitigs && !counts_out), nullptr, nullptr, &device, err, errlen)) return orc;
    if (n_positive) *n_positive = 0;
    fin_hits* h = nullptr;
    int rc = fin_hits_create(idx, device, &h, err, errlen);
    if (rc != FIN_OK) return rc;
    rc = fin_search_batch_add_hits(idx, bases, offsets, n_reads, strands, h, err, errlen);
    if (rc == FIN_OK) rc = fin_hits_download(h, counts_out, n_positive, err, errlen);
    fin_hits_free(h);
    return rc;
}

int fin_search_batch_add_cover(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, fin_cover* c, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, c, c, OTHER_ACC, &device, err, errlen)) return orc;
    if (n_reads == 0) return FIN_OK;
    Product p;
    p.take = [&](fin_batch* b, const SubBatch&, uint64_t&, char* e, size_t elen) -> int { return fin_batch_add_cover(b, c, own(b), e, elen); };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, nullptr, err, errlen);
}

int fin_search_batch_unitig_coverage(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, uint64_t* covered_out,
                                     uint64_t* n_positive, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, !(idx && idx->n_unitigs && !covered_out), nullptr, nullptr, &device, err, errlen)) return orc;
    if (n_positive) *n_positive = 0;
    fin_cover* c = nullptr;
    fin_hits* h = nullptr;   // the found k-mers are a sum of depths, which the bitmap does not hold: asked for, they come from a profile added behind the same runs
    int rc = fin_cover_create(idx, device, &c, err, errlen);
    if (rc == FIN_OK && n_positive) rc = fin_hits_create(idx, device, &h, err, errlen);
    if (rc == FIN_OK && n_reads) {
        Product p;   // both adds go behind the same run
        p.take = [&](fin_batch* b, const SubBatch&, uint64_t&, char* e, size_t elen) -> int {
            if (h) if (const int hrc = fin_batch_add_hits(b, h, own(b), e, elen)) return hrc;
            return fin_batch_add_cover(b, c, own(b), e, elen);
        };
        rc = search_product(idx, device, bases, offsets, n_reads, strands, p, nullptr, err, errlen);
    }
    if (rc == FIN_OK) rc = fin_cover_download(c, nullptr, covered_out, nullptr, err, errlen);
    if (rc == FIN_OK && h) rc = fin_hits_download(h, nullptr, n_positive, err, errlen);
    fin_hits_free(h); fin_cover_free(c);
    return rc;
}

int fin_search_batch_add_depth(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, fin_depth* d, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, d, d, OTHER_ACC, &device, err, errlen)) return orc;
    if (n_reads == 0) return FIN_OK;
    Product p;
    p.take = [&](fin_batch* b, const SubBatch&, uint64_t&, char* e, size_t elen) -> int { return fin_batch_add_depth(b, d, own(b), e, elen); };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, nullptr, err, errlen);
}

int fin_search_batch_unitig_depth(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, uint32_t min_depth,
                                  fin_depth_stat* stats_out, uint64_t* n_positive, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, !(idx && idx->n_unitigs && !stats_out), nullptr, nullptr, &device, err, errlen)) return orc;
    if (n_positive) *n_positive = 0;
    fin_depth* d = nullptr;
    int rc = fin_depth_create(idx, device, &d, err, errlen);
    if (rc != FIN_OK) return rc;
    rc = fin_search_batch_add_depth(idx, bases, offsets, n_reads, strands, d, err, errlen);
    if (rc == FIN_OK) rc = fin_depth_download(d, min_depth, nullptr, stats_out, n_positive, err, errlen);   // (the found k-mers are the sum of the depths)
    fin_depth_free(d);
    return rc;
}

int fin_search_batch_add_pileup(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, fin_pileup* pl, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, pl, pl, OTHER_ACC, &device, err, errlen)) return orc;
    if (n_reads == 0) return FIN_OK;
    Product p;
    p.take = [&](fin_batch* b, const SubBatch&, uint64_t&, char* e, size_t elen) -> int { return fin_batch_add_pileup(b, pl, own(b), e, elen); };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, nullptr, err, errlen);
}

int fin_search_batch_add_fragments(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, fin_fragments* f, char* err,
                                   size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, f, f, OTHER_ACC, &device, err, errlen)) return orc;
    if (const int crc = check_even_fragments(n_reads, err, errlen)) return crc;
    if (n_reads == 0) return FIN_OK;
    Product p; p.group = 2;   // (interleaved mates: no sub-batch splits a pair)
    p.take = [&](fin_batch* b, const SubBatch&, uint64_t&, char* e, size_t elen) -> int { return fin_batch_add_fragments(b, f, own(b), e, elen); };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, nullptr, err, errlen);
}

int fin_search_batch_fragments(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, fin_fragment* frags_out, char* err,
                               size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, n_reads < 2 || frags_out, nullptr, nullptr, &device, err, errlen)) return orc;
    if (const int crc = check_even_fragments(n_reads, err, errlen)) return crc;
    if (n_reads == 0) return FIN_OK;
    Product p; p.group = 2;   // a sub-batch's fragments land at the fragments' numbers (every sub-batch begins at an even read)
    p.take = [&](fin_batch* b, const SubBatch& s, uint64_t&, char* e, size_t elen) -> int {
        if (const int rc = fin_batch_fragments(b, nullptr, e, elen)) return rc;
        return fin_batch_download_fragments(b, frags_out + s.lo / 2, e, elen);
    };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, nullptr, err, errlen);
}

int fin_search_batch_add_links(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands, fin_links* l, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, strands, l, l, OTHER_ACC, &device, err, errlen)) return orc;
    if (n_reads == 0) return FIN_OK;
    Product p;   // (no sub-batch cuts a read: nothing is lost between them)
    p.take = [&](fin_batch* b, const SubBatch&, uint64_t&, char* e, size_t elen) -> int { return fin_batch_add_links(b, l, own(b), e, elen); };
    return search_product(idx, device, bases, offsets, n_reads, strands, p, nullptr, err, errlen);
}

// ---- reference coordinates: depth and variant candidates lifted onto sequences (fin_refpaths.hip) ---------------------------------------------
// The sequences' tables are small and live on the host (seq_nk, seg_offs); the segments lie in HBM alone.  seg_offs goes to the device when a kernel or a caller
// wants it.  `mu` guards everything but `pend`
struct fin_refpaths : fin_acc {
    uint64_t n_unitigs = 0, total_len = 0;
    const uint32_t* d_ends = nullptr;     // the replica's ends_p
    std::mutex mu;
    std::vector<uint32_t> seq_nk;         // [n_seqs]
    std::vector<uint64_t> seg_offs{0};    // [n_seqs + 1]
    uint64_t n_slots = 0;
    void* d_segs = nullptr; size_t cap_segs = 0;         // fin_segment[n_segments], room for cap_segs of them
    void* d_seg_offs = nullptr; size_t cap_offs = 0;     // uint64[n_seqs + 1] where offs_fresh
    bool offs_fresh = false;
    uint32_t* d_ctl = nullptr;            // 16 bytes: what a reset zeroes (the appends are ordered against it), word 0 the flag word of a call, words 2 and 3 a call's uint64 total
};
static_assert(sizeof(fin_ref_window) == 16 && sizeof(fin_ref_variant) == 16 && sizeof(fin_variant) == 32, "the kernels' 16- and 32-byte entries");
static const char* const REFPATHS_OUTSIDE = "a segment outside the index was met: nothing was written (reset the path set)";
namespace {
struct DevMem {   // a call's own allocation, freed on every way out
    void* p = nullptr;
    ~DevMem() { if (p) (void)hipFree(p); }
    bool get(size_t bytes) { if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return false; } return true; }
};
}  // namespace
static uint64_t refpaths_n_segs(const fin_refpaths* rp) { return rp->seg_offs.back(); }
// room for n segments, what is there kept (with mu held)
static int refpaths_room(fin_refpaths* rp, uint64_t n, char* err, size_t errlen) {
    if (n <= rp->cap_segs) return FIN_OK;
    if (const int wrc = rp->pend.wait(err, errlen)) return wrc;
    const size_t want = (size_t)(n + n / 4 + 1024);
    void* p = nullptr;
    if (hipMalloc(&p, want * 16) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "out of device memory (reference paths)"); return FIN_ENOMEM; }
    const uint64_t have = refpaths_n_segs(rp);
    if (have && hipMemcpy(p, rp->d_segs, (size_t)have * 16, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipFree(p); set_err(err, errlen, "hipMemcpy failed"); return FIN_ENODEV; }
    (void)hipFree(rp->d_segs);
    rp->d_segs = p; rp->cap_segs = want;
    return FIN_OK;
}
// seg_offs on the device, on the null stream (with mu held)
static int refpaths_offs(fin_refpaths* rp, char* err, size_t errlen) {
    if (rp->offs_fresh) return FIN_OK;
    const size_t n = rp->seg_offs.size();
    if (n > rp->cap_offs) {
        (void)hipFree(rp->d_seg_offs); rp->d_seg_offs = nullptr; rp->cap_offs = 0;
        if (hipMalloc(&rp->d_seg_offs, (n + n / 4 + 64) * 8) != hipSuccess) { (void)hipGetLastError(); rp->d_seg_offs = nullptr; set_err(err, errlen, "out of device memory (reference paths)"); return FIN_ENOMEM; }
        rp->cap_offs = n + n / 4 + 64;
    }
    HIPCHK(hipMemcpy(rp->d_seg_offs, rp->seg_offs.data(), n * 8, hipMemcpyHostToDevice));
    rp->offs_fresh = true;
    return FIN_OK;
}

void fin_refpaths_free(fin_refpaths* rp) {
    if (!acc_free_open(rp)) return;
    (void)hipFree(rp->d_segs); (void)hipFree(rp->d_seg_offs); (void)hipFree(rp->d_ctl);
    delete rp;
}

int fin_refpaths_create(const fin_index* idx, int device, fin_refpaths** out, char* err, size_t errlen) {
    if (!idx || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    *out = nullptr;
    const fin_index::Replica* rep = nullptr;
    if (const int orc = acc_create_open(idx, device, &rep, err, errlen)) return orc;
    fin_refpaths* rp = acc_new<fin_refpaths>(idx, device, err, errlen);
    if (!rp) return FIN_ENOMEM;
    rp->n_unitigs = idx->n_unitigs; rp->total_len = idx->total_len; rp->d_ends = rep->dev.ends;
    if (const int arc = acc_alloc_zero(rp, (void**)&rp->d_ctl, 16, 16, "out of device memory (reference paths)", fin_refpaths_free, err, errlen)) return arc;
    *out = rp;
    return FIN_OK;
}

int fin_refpaths_reset(fin_refpaths* rp, void* hip_stream) {
    if (!rp) return FIN_EINVAL;
    std::lock_guard<std::mutex> g(rp->mu);
    rp->seq_nk.clear(); rp->seg_offs.assign(1, 0); rp->n_slots = 0; rp->offs_fresh = false;
    return acc_reset(rp, hip_stream, rp->d_ctl, 16);
}

uint64_t fin_refpaths_n_seqs(const fin_refpaths* rp) { if (!rp) return 0; std::lock_guard<std::mutex> g(const_cast<fin_refpaths*>(rp)->mu); return rp->seq_nk.size(); }
uint64_t fin_refpaths_n_segments(const fin_refpaths* rp) { if (!rp) return 0; std::lock_guard<std::mutex> g(const_cast<fin_refpaths*>(rp)->mu); return refpaths_n_segs(rp); }
uint64_t fin_refpaths_n_slots(const fin_refpaths* rp) { if (!rp) return 0; std::lock_guard<std::mutex> g(const_cast<fin_refpaths*>(rp)->mu); return rp->n_slots; }
void* fin_refpaths_device_segments(const fin_refpaths* rp) { return rp ? rp->d_segs : nullptr; }
void* fin_refpaths_device_segment_offsets(fin_refpaths* rp) {
    if (!rp || hipSetDevice(rp->device) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> g(rp->mu);
    return refpaths_offs(rp, nullptr, 0) == FIN_OK ? rp->d_seg_offs : nullptr;
}

int fin_refpaths_download(fin_refpaths* rp, uint32_t* seq_nk_out, uint64_t* seg_offs_out, fin_segment* segs_out, char* err, size_t errlen) {
    if (!rp) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (const int orc = acc_download_open(rp, nullptr, nullptr, nullptr, err, errlen)) return orc;
    std::lock_guard<std::mutex> g(rp->mu);
    if (seq_nk_out && !rp->seq_nk.empty()) memcpy(seq_nk_out, rp->seq_nk.data(), rp->seq_nk.size() * 4);
    if (seg_offs_out) memcpy(seg_offs_out, rp->seg_offs.data(), rp->seg_offs.size() * 8);
    if (segs_out && refpaths_n_segs(rp)) HIPCHK(hipMemcpy(segs_out, rp->d_segs, (size_t)refpaths_n_segs(rp) * 16, hipMemcpyDeviceToHost));
    return FIN_OK;
}

// unitigs.ends as FIN_X_ENDS has them, from the index's starts
static std::vector<int64_t> refpaths_host_ends(const fin_index* idx) {
    std::vector<int64_t> e((size_t)idx->n_unitigs);
    for (uint64_t u = 0; u < idx->n_unitigs; u++) e[(size_t)u] = (int64_t)idx->ends[u + 1];
    return e;
}

int fin_refpaths_upload(fin_refpaths* rp, const uint32_t* seq_nk, const uint64_t* seg_offs, const fin_segment* segs, uint64_t n_seqs, char* err, size_t errlen) {
    if (!rp || (n_seqs && (!seq_nk || !seg_offs))) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    const std::vector<int64_t> ends = refpaths_host_ends(rp->idx);
    if (const int crc = fin_segments_check(seq_nk, seg_offs, segs, n_seqs, (int)rp->idx->k, ends.data(), rp->n_unitigs, err, errlen)) return crc;
    HIPCHK(hipSetDevice(rp->device));
    if (const int wrc = rp->pend.wait(err, errlen)) return wrc;
    std::lock_guard<std::mutex> g(rp->mu);
    const uint64_t n = n_seqs ? seg_offs[n_seqs] : 0;
    if (n > rp->cap_segs) {   // (nothing is kept: the contents are replaced)
        void* p = nullptr;
        if (hipMalloc(&p, (size_t)n * 16) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "out of device memory (reference paths)"); return FIN_ENOMEM; }
        (void)hipFree(rp->d_segs);
        rp->d_segs = p; rp->cap_segs = (size_t)n;
    }
    if (n) HIPCHK(hipMemcpy(rp->d_segs, segs, (size_t)n * 16, hipMemcpyHostToDevice));
    rp->seq_nk.assign(seq_nk, seq_nk + n_seqs);
    if (n_seqs) rp->seg_offs.assign(seg_offs, seg_offs + n_seqs + 1); else rp->seg_offs.assign(1, 0);
    rp->n_slots = sum_of(seq_nk, (size_t)n_seqs, [](uint32_t v) { return v; });
    rp->offs_fresh = false;
    return FIN_OK;
}

// the batch's segments as they lie in HBM, made if there are none, and its seg_offs on the host: everything the segment kernels were given has finished
static int refpaths_batch_segments(fin_batch* b, std::vector<uint64_t>& so, char* err, size_t errlen) {
    if (!b->sgm_ready) if (const int rc = fin_batch_segments(b, nullptr, err, errlen)) return rc;
    so.resize((size_t)b->n_reads + 1);
    HIPCHK(hipMemcpyAsync(so.data(), b->d_sgm_offs, so.size() * 8, hipMemcpyDeviceToHost, b->last_stream));
    HIPCHK(hipStreamSynchronize(b->last_stream));
    if (so[0] != 0 || so.back() != b->n_segments) { set_err(err, errlen, "segment kernels: offsets and count disagree"); return FIN_ENODEV; }
    return FIN_OK;
}
// the sequences of one batch behind those that are there (with mu held): the tables on the host, the segments from `src` device to device on `st`
static int refpaths_append(fin_refpaths* rp, const fin_batch* b, const std::vector<uint64_t>& so, const void* src, hipStream_t st, char* err, size_t errlen) {
    const uint64_t have = refpaths_n_segs(rp), L = so.back();
    if (const int rrc = refpaths_room(rp, have + L, err, errlen)) return rrc;
    if (L) HIPCHK(hipMemcpyAsync((char*)rp->d_segs + (size_t)have * 16, src, (size_t)L * 16, hipMemcpyDeviceToDevice, st));
    for (uint64_t r = 0; r < b->n_reads; r++) {
        const uint32_t nk = (uint32_t)(b->h_out_offs[r + 1] - b->h_out_offs[r]);
        rp->seq_nk.push_back(nk); rp->n_slots += nk;
        rp->seg_offs.push_back(have + so[(size_t)r + 1]);
    }
    rp->offs_fresh = false;
    return FIN_OK;
}

int fin_batch_add_refpaths(fin_batch* b, fin_refpaths* rp, void* hip_stream, char* err, size_t errlen) {
    if (!b || !rp) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    hipStream_t st = (hipStream_t)hip_stream;
    if (const int orc = acc_add_open(b, rp, st, err, errlen)) return orc;
    std::vector<uint64_t> so;
    if (const int src = refpaths_batch_segments(b, so, err, errlen)) return src;
    std::lock_guard<std::mutex> g(rp->mu);
    if (const int arc = refpaths_append(rp, b, so, b->d_sgm, st, err, errlen)) return arc;
    return acc_add_close(rp, st, 0, "", err, errlen);
}

int fin_search_batch_add_refpaths(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, fin_refpaths* rp, char* err, size_t errlen) {
    int device = -1;
    if (const int orc = search_open(idx, offsets, FIN_MERGED, rp, rp, OTHER_ACC, &device, err, errlen)) return orc;
    if (n_reads == 0) return FIN_OK;
    // Sub-batches finish in any order and the sequences are appended in the reads': each worker copies its segments device to device into a buffer of its own,
    // and they are put behind one another once all are there.  Nobody waits for anybody, so a worker that fails strands no other
    struct Part { size_t i; std::vector<uint32_t> nk; std::vector<uint64_t> so; void* d = nullptr; };
    std::mutex pmu;
    std::vector<Part> parts;
    Product p;
    p.take = [&](fin_batch* b, const SubBatch& s, uint64_t&, char* e, size_t elen) -> int {
        Part q; q.i = s.i;
        if (const int rc = refpaths_batch_segments(b, q.so, e, elen)) return rc;
        const uint64_t L = q.so.back();
        if (L) {
            if (hipMalloc(&q.d, (size_t)L * 16) != hipSuccess) { (void)hipGetLastError(); snprintf(e, elen, "out of device memory (reference paths)"); return FIN_ENOMEM; }
            if (hipMemcpy(q.d, b->d_sgm, (size_t)L * 16, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipFree(q.d); snprintf(e, elen, "hipMemcpy failed"); return FIN_ENODEV; }
        }
        q.nk.resize((size_t)b->n_reads);
        for (uint64_t r = 0; r < b->n_reads; r++) q.nk[(size_t)r] = (uint32_t)(b->h_out_offs[r + 1] - b->h_out_offs[r]);
        std::lock_guard<std::mutex> g(pmu);
        parts.push_back(std::move(q));
        return FIN_OK;
    };
    int rc = search_product(idx, device, bases, offsets, n_reads, FIN_MERGED, p, nullptr, err, errlen);
    if (rc == FIN_OK && hipSetDevice(device) != hipSuccess) { set_err(err, errlen, "hipSetDevice failed"); rc = FIN_ENODEV; }
    if (rc == FIN_OK) {
        std::sort(parts.begin(), parts.end(), [](const Part& a, const Part& b) { return a.i < b.i; });
        uint64_t more = 0;
        for (const Part& q : parts) more += q.so.back();
        std::lock_guard<std::mutex> g(rp->mu);
        rc = refpaths_room(rp, refpaths_n_segs(rp) + more, err, errlen);
        for (size_t j = 0; rc == FIN_OK && j < parts.size(); j++) {
            const Part& q = parts[j];
            const uint64_t have = refpaths_n_segs(rp), L = q.so.back();
            if (L && hipMemcpy((char*)rp->d_segs + (size_t)have * 16, q.d, (size_t)L * 16, hipMemcpyDeviceToDevice) != hipSuccess) { set_err(err, errlen, "hipMemcpy failed"); rc = FIN_ENODEV; break; }
            for (size_t r = 0; r < q.nk.size(); r++) { rp->seq_nk.push_back(q.nk[r]); rp->n_slots += q.nk[r]; rp->seg_offs.push_back(have + q.so[r + 1]); }
            rp->offs_fresh = false;
        }
    }
    for (Part& q : parts) (void)hipFree(q.d);
    return rc;
}

int fin_refpaths_depth(fin_refpaths* rp, fin_depth* dep, uint32_t window, uint32_t min_depth, uint64_t* win_offs_out, fin_ref_window* out, uint64_t cap,
                       uint64_t* n_windows, char* err, size_t errlen) {
    if (n_windows) *n_windows = 0;
    if (!rp || !dep) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    if (window == 0) { set_err(err, errlen, "window is at least 1"); return FIN_EINVAL; }
    if (dep->idx != rp->idx || dep->device != rp->device) { set_err(err, errlen, "paths and depth accumulator belong to different indexes or devices"); return FIN_EINVAL; }
    // the two waits, with the downloads' own codes and messages for a withheld step or a pair outside the index (nothing else happens in these calls)
    if (const int rc = fin_refpaths_download(rp, nullptr, nullptr, nullptr, err, errlen)) return rc;
    if (const int rc = fin_depth_download(dep, min_depth, nullptr, nullptr, nullptr, err, errlen)) return rc;
    std::lock_guard<std::mutex> g(rp->mu);
    const uint64_t n_seqs = rp->seq_nk.size(), n_segs = refpaths_n_segs(rp);
    std::vector<uint64_t> wo((size_t)n_seqs + 1, 0);
    for (uint64_t s = 0; s < n_seqs; s++) wo[(size_t)s + 1] = wo[(size_t)s] + ((uint64_t)rp->seq_nk[(size_t)s] + window - 1) / window;
    const uint64_t W = wo[(size_t)n_seqs];
    if (n_windows) *n_windows = W;
    if (W > cap || (W && !out)) { set_err(err, errlen, "window buffer too small: room for " + std::to_string(cap) + " windows, " + std::to_string(W) + " needed"); return FIN_ELIMIT; }
    if (W == 0 || n_segs == 0 || rp->total_len == 0) {   // nothing lies in the graph
        if (win_offs_out) memcpy(win_offs_out, wo.data(), wo.size() * 8);
        if (W) memset(out, 0, (size_t)W * sizeof(fin_ref_window));
        return FIN_OK;
    }
    if (const int orc = refpaths_offs(rp, err, errlen)) return orc;
    // the call's own memory: the depths of the whole text; then the windows, their offsets, and the tiles' tables
    const uint32_t tile = fin_rp_tile((uint32_t)optv(rp->idx, O_refpaths_tile)), nb = fin_rp_blocks(n_segs);
    DevMem full, aux;
    const size_t b_win = (size_t)W * 16, b_wo = wo.size() * 8, b_toffs = ((size_t)n_segs + 1) * 8, b_boff = ((size_t)nb + 1) * 8, b_cnt = ((size_t)n_segs + 4) / 4 * 16,
                 b_bsum = ((size_t)nb + 4) / 4 * 16;
    if (!full.get((size_t)rp->total_len * 4) || !aux.get(b_win + b_wo + b_toffs + b_boff + b_cnt + b_bsum)) { set_err(err, errlen, "out of device memory (reference depth)"); return FIN_ENOMEM; }
    char* const a = (char*)aux.p;
    void* const d_win = a;
    uint64_t* const d_wo = (uint64_t*)(a + b_win);
    uint64_t* const d_toffs = (uint64_t*)(a + b_win + b_wo);
    uint64_t* const d_boff = (uint64_t*)(a + b_win + b_wo + b_toffs);
    uint32_t* const d_cnt = (uint32_t*)(a + b_win + b_wo + b_toffs + b_boff);
    uint32_t* const d_bsum = (uint32_t*)(a + b_win + b_wo + b_toffs + b_boff + b_cnt);
    uint64_t* const d_total = (uint64_t*)(rp->d_ctl + 2);
    {   // everything below is on the null stream; the lock keeps a download from scanning in between
        std::lock_guard<std::mutex> gd(dep->scan_mu);
        const int rc = depth_scan(dep, min_depth, nullptr, false, err, errlen, [&](uint64_t base, uint64_t n) {
            return (int)hipMemcpyAsync((uint32_t*)full.p + base, dep->d_stage, (size_t)n * 4, hipMemcpyDeviceToDevice, nullptr);
        });
        if (rc) return rc;
    }
    HIPCHK(hipMemsetAsync(d_win, 0, b_win, nullptr));
    HIPCHK(hipMemsetAsync(rp->d_ctl, 0, 16, nullptr));
    HIPCHK(hipMemcpyAsync(d_wo, wo.data(), b_wo, hipMemcpyHostToDevice, nullptr));
    int krc = fin_launch_rp_tiles(rp->d_segs, n_segs, tile, d_cnt, d_bsum, d_boff, d_toffs, d_total, nullptr);
    uint64_t n_tiles = 0;
    if (krc == 0) {
        HIPCHK(hipMemcpy(&n_tiles, d_total, 8, hipMemcpyDeviceToHost));
        krc = fin_launch_rp_depth(rp->d_segs, n_segs, (const uint64_t*)rp->d_seg_offs, n_seqs, d_toffs, n_tiles, tile, d_wo, window, min_depth, (const uint32_t*)full.p,
                                  rp->d_ends, (uint32_t)rp->n_unitigs, rp->total_len, rp->idx->k, d_win, rp->d_ctl, nullptr);
    }
    if (krc != 0) { set_err(err, errlen, std::string("reference depth kernels: ") + hipGetErrorString((hipError_t)krc)); return FIN_ENODEV; }
    uint32_t flags = 0;
    HIPCHK(hipMemcpy(&flags, rp->d_ctl, 4, hipMemcpyDeviceToHost));   // (the null stream: behind the kernels)
    if (flags) { set_err(err, errlen, REFPATHS_OUTSIDE); return FIN_EINVAL; }
    HIPCHK(hipMemcpy(out, d_win, b_win, hipMemcpyDeviceToHost));
    if (win_offs_out) memcpy(win_offs_out, wo.data(), wo.size() * 8);
    return FIN_OK;
}

int fin_refpaths_lift_variants(fin_refpaths* rp, const fin_variant* vars, uint64_t n, fin_ref_variant* out, uint64_t cap, uint64_t* n_out, char* err, size_t errlen) {
    if (n_out) *n_out = 0;
    if (!rp || (n && !vars)) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    // the variants, on the host: inside the index, strictly ascending
    const fin_index* idx = rp->idx;
    uint64_t prev = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (vars[i].u >= idx->n_unitigs || (uint64_t)idx->ends[vars[i].u] + vars[i].off >= idx->ends[vars[i].u + 1]) { set_err(err, errlen, "variant " + std::to_string(i) + " lies outside the index"); return FIN_EINVAL; }
        const uint64_t g = (uint64_t)idx->ends[vars[i].u] + vars[i].off;
        if (i && g <= prev) { set_err(err, errlen, "variant " + std::to_string(i) + " does not ascend: the variants are strictly ascending in start(u) + off"); return FIN_EINVAL; }
        prev = g;
    }
    if (const int rc = fin_refpaths_download(rp, nullptr, nullptr, nullptr, err, errlen)) return rc;
    std::lock_guard<std::mutex> g(rp->mu);
    const uint64_t n_seqs = rp->seq_nk.size(), n_segs = refpaths_n_segs(rp);
    if (n_segs == 0) return FIN_OK;   // (with no variant the segments are still looked at: the guard)
    if (const int orc = refpaths_offs(rp, err, errlen)) return orc;
    const uint32_t nb = fin_rp_blocks(n_segs);
    DevMem aux, rec;
    const size_t b_vars = (size_t)n * 32, b_g = (size_t)n * 8 + 8, b_boff = ((size_t)nb + 1) * 8, b_cnt = ((size_t)n_segs + 4) / 4 * 16, b_bsum = ((size_t)nb + 4) / 4 * 16;
    if (!aux.get(b_vars + b_g + b_boff + b_cnt + b_bsum)) { set_err(err, errlen, "out of device memory (lifted variants)"); return FIN_ENOMEM; }
    char* const a = (char*)aux.p;
    uint64_t* const d_g = (uint64_t*)(a + b_vars);
    uint64_t* const d_boff = (uint64_t*)(a + b_vars + b_g);
    uint32_t* const d_cnt = (uint32_t*)(a + b_vars + b_g + b_boff);
    uint32_t* const d_bsum = (uint32_t*)(a + b_vars + b_g + b_boff + b_cnt);
    uint64_t* const d_total = (uint64_t*)(rp->d_ctl + 2);
    const uint32_t nu = (uint32_t)rp->n_unitigs, k = idx->k;
    if (n) HIPCHK(hipMemcpyAsync(a, vars, b_vars, hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemsetAsync(rp->d_ctl, 0, 16, nullptr));
    int krc = fin_launch_rp_var_g(a, n, rp->d_ends, d_g, nullptr);
    if (krc == 0) krc = fin_launch_rp_var_count(rp->d_segs, n_segs, d_g, n, rp->d_ends, nu, rp->total_len, k, d_cnt, d_bsum, d_boff, d_total, rp->d_ctl, nullptr);
    if (krc != 0) { set_err(err, errlen, std::string("variant lift kernels: ") + hipGetErrorString((hipError_t)krc)); return FIN_ENODEV; }
    uint32_t ctl[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(ctl, rp->d_ctl, 16, hipMemcpyDeviceToHost));   // (the null stream: behind the kernels)
    if (ctl[0]) { set_err(err, errlen, REFPATHS_OUTSIDE); return FIN_EINVAL; }
    const uint64_t total = ((uint64_t)ctl[3] << 32) | ctl[2];
    if (n_out) *n_out = total;
    if (total > cap || (total && !out)) { set_err(err, errlen, "record buffer too small: room for " + std::to_string(cap) + " records, " + std::to_string(total) + " needed"); return FIN_ELIMIT; }
    if (total == 0) return FIN_OK;
    if (!rec.get((size_t)total * 16)) { set_err(err, errlen, "out of device memory (lifted variants)"); return FIN_ENOMEM; }
    krc = fin_launch_rp_var_write(rp->d_segs, n_segs, (const uint64_t*)rp->d_seg_offs, n_seqs, d_g, n, rp->d_ends, nu, rp->total_len, k, d_boff, rec.p, rp->d_ctl, nullptr);
    if (krc != 0) { set_err(err, errlen, std::string("variant lift kernels: ") + hipGetErrorString((hipError_t)krc)); return FIN_ENODEV; }
    HIPCHK(hipMemcpy(out, rec.p, (size_t)total * 16, hipMemcpyDeviceToHost));
    return FIN_OK;
}

int fin_search_batch(const fin_index* idx, const char* bases, const uint64_t* offsets, uint64_t n_reads, int strands,
                     int32_t* pairs_out, uint64_t* n_positive, char* err, size_t errlen) {
    if (!idx || !offsets) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    int device = -1;
    if (const int orc = search_home(idx, nullptr, nullptr, &device, err, errlen)) return orc;
    if (n_positive) *n_positive = 0;
    return search_range_on(idx, device, bases, offsets, 0, n_reads, strands, pairs_out, n_positive, err, errlen);
}

int fin_search_batch_multi(fin_index* idx, const int* devices, int n_devices, const char* bases, const uint64_t* offsets,
                           uint64_t n_reads, int strands, int32_t* pairs_out, uint64_t* n_positive, char* err, size_t errlen) {
    if (!idx || !offsets || !devices || n_devices < 1) { set_err(err, errlen, "bad argument"); return FIN_EINVAL; }
    for (int d = 0; d < n_devices; d++) { int rc = fin_index_to_device(idx, devices[d], err, errlen); if (rc) return rc; }
    if (n_positive) *n_positive = 0;
    // contiguous shards of read records balanced by bases: per-device outputs concatenate in input order
    const uint64_t k = idx->k;
    std::vector<uint64_t> cut((size_t)n_devices + 1, n_reads), pair_at((size_t)n_devices + 1, 0);
    cut[0] = 0;
    const uint64_t total = offsets[n_reads] - offsets[0];
    uint64_t r = 0, pairs = 0;
    for (int d = 1; d <= n_devices; d++) {
        const uint64_t target = d == n_devices ? total : total / (uint64_t)n_devices * (uint64_t)d;
        while (r < n_reads && (offsets[r] - offsets[0] < target || d == n_devices)) {
            const uint64_t len = offsets[r + 1] - offsets[r];
            pairs += len >= k ? len - k + 1 : 0; r++;
        }
        cut[(size_t)d] = r; pair_at[(size_t)d] = pairs;
    }
    std::vector<int> rcs((size_t)n_devices, FIN_OK);
    std::vector<uint64_t> pos((size_t)n_devices, 0);
    std::vector<std::string> errs((size_t)n_devices);
    std::vector<std::thread> th;
    for (int d = 0; d < n_devices; d++) {
        th.emplace_back([&, d]() {
            char e[512] = {0};
            if (cut[(size_t)d + 1] > cut[(size_t)d])
                rcs[(size_t)d] = search_range_on(idx, devices[d], bases, offsets, cut[(size_t)d], cut[(size_t)d + 1], strands,
                                                 pairs_out ? pairs_out + 2 * pair_at[(size_t)d] : nullptr, &pos[(size_t)d], e, sizeof e);
            errs[(size_t)d] = e;
        });
    }
    for (auto& t : th) t.join();
    uint64_t tot = 0;
    for (int d = 0; d < n_devices; d++) {
        if (rcs[(size_t)d] != FIN_OK) { set_err(err, errlen, "device " + std::to_string(devices[d]) + ": " + errs[(size_t)d]); return rcs[(size_t)d]; }
        tot += pos[(size_t)d];
    }
    if (n_positive) *n_positive = tot;
    return FIN_OK;
}

void* fin_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void fin_host_free(void* p) { if (p) (void)hipHostFree(p); }

int fin_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int fin_search(const fin_index* idx, const char* seq, int64_t len, int64_t* pairs_out, int64_t* n_found, char* err, size_t errlen) {
    if (!idx || len < 0 || (len && !seq)) { set_err(err, errlen, "bad argument"); return FIN_EINVAL; }
    uint64_t offs[2] = {0, (uint64_t)len};
    int64_t nk = len - (int64_t)idx->k + 1; if (nk < 0) nk = 0;
    std::vector<int32_t> tmp((size_t)(2 * nk + 2));
    int rc = fin_search_batch(idx, seq ? seq : "", offs, 1, FIN_FWD, tmp.data(), nullptr, err, errlen);
    if (rc) return rc;
    int64_t nf = 0;
    for (int64_t i = 0; i < nk; i++) {
        if (pairs_out) { pairs_out[2 * i] = tmp[2 * i]; pairs_out[2 * i + 1] = tmp[2 * i + 1]; }
        nf += tmp[2 * i] != -1;
    }
    if (n_found) *n_found = nf;
    return FIN_OK;
}

int64_t fin_format_pairs(const int32_t* pairs, int64_t n_pairs, char* out) {
    char* p = out;
    for (int64_t i = 0; i < n_pairs; i++) {
        if (i) *p++ = ' ';
        *p++ = '(';
        for (int h = 0; h < 2; h++) {
            int64_t v = pairs[2 * i + h];
            if (v < 0) { *p++ = '-'; v = -v; }
            char tmp[16]; int n = 0;
            do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
            while (n) *p++ = tmp[--n];
            *p++ = h == 0 ? ',' : ')';
        }
    }
    *p++ = '\n';
    return (int64_t)(p - out);
}


// ---- index sets: a unitig set beyond 2^32 nodes as PARTS (round 5; VERDICT r4 missing #1) ---------------------------------------------------------------
// The reference is int64_t throughout (common.hh:79-93, FinimizerIndex.hh:30-33); this build's node numbers and text offsets are u32 in every device
// structure, so ONE index stops at 2^32 nodes (a 4.1 Gbp unitig set: 4.12e9 nodes).  A set splits the input unitigs, in input order, into
// parts of at most max_part_bases bases, builds an ordinary index of each and searches a read in every part: a k-mer of a disjoint spectrum-preserving string
// set -- what the reference requires as input (README.md:79-80) -- lies in ONE unitig, hence in one part, and is reported there at the offset the whole
// index would report; the part's unitig number is mapped to the number permute_unitigs (PackedStrings.hh:105-135) gives that unitig in the whole set
// (rank of its first k-mer in colex order, ties by input order: the parts' orders are that order restricted to their unitigs).  What makes the set EXACT is
// checked when it is built (verify != 0): no part holds a k-mer twice (fin_index_is_disjoint), and no k-mer of one part occurs, on either strand, in
// another -- every part's unitigs are searched in the parts behind it; a set that fails is refused (FIN_EINVAL): which occurrence of a shared k-mer the
// reference reports is decided by its finimizers' stored offsets over the WHOLE index, which no part knows.  Cost: the parts' steps one after the other
// and a merge pass each (fin_set_merge_kernel).
struct fin_pindex {
    int k = 0, device = -1;
    std::vector<fin_index*> parts;
    std::vector<uint64_t> first_unitig;            // part p holds input unitigs [first_unitig[p], first_unitig[p+1])
    std::vector<std::vector<uint32_t>> gid;        // per part: its unitig number -> the set's
    std::vector<uint32_t*> d_gid;
    uint64_t n_unitigs = 0;
    int64_t shared_kmers = -1;                     // k-mers found in a part other than their own at build (-1: not checked)
    double verify_s = 0.0;
    // fin_pindex_search_batch keeps its device batches from call to call (a caller that streams chunks of reads through it allocates once)
    mutable std::mutex mu; mutable struct fin_pbatch* cached = nullptr;
    // Lifetime: the owner holds one reference and every fin_pbatch one (its parts' batches live on the set's fin_index handles and its merge reads d_gid), so
    // fin_pindex_free and fin_pbatch_free may come in either order; whoever drops the last reference destroys the set.
    mutable std::atomic<int> refs{1};
};
void fin_pbatch_free(fin_pbatch* sb);

static void pindex_release(const fin_pindex* cs) {
    if (!cs || cs->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
    fin_pindex* s = const_cast<fin_pindex*>(cs);
    if (s->device >= 0) (void)hipSetDevice(s->device);
    for (uint32_t* g : s->d_gid) (void)hipFree(g);
    for (fin_index* p : s->parts) fin_index_free(p);
    delete s;
}
// the owner's reference.  The cached batch of fin_pindex_search_batch is the owner's too: it goes here (with its reference), or it would keep the set alive
void fin_pindex_free(fin_pindex* s) {
    if (!s) return;
    fin_pbatch* c = nullptr;
    { std::lock_guard<std::mutex> g(s->mu); c = s->cached; s->cached = nullptr; }
    fin_pbatch_free(c);
    pindex_release(s);
}
uint32_t fin_pindex_parts(const fin_pindex* s) { return s ? (uint32_t)s->parts.size() : 0u; }
const fin_index* fin_pindex_part(const fin_pindex* s, uint32_t p) { return (s && p < s->parts.size()) ? s->parts[p] : nullptr; }
int64_t fin_pindex_k(const fin_pindex* s) { return s ? s->k : -1; }
int64_t fin_pindex_n_unitigs(const fin_pindex* s) { return s ? (int64_t)s->n_unitigs : -1; }
int64_t fin_pindex_shared_kmers(const fin_pindex* s) { return s ? s->shared_kmers : -1; }
double fin_pindex_verify_seconds(const fin_pindex* s) { return s ? s->verify_s : 0.0; }
static int64_t set_sum(const fin_pindex* s, int64_t (*f)(const fin_index*)) {
    if (!s) return -1;
    int64_t t = 0;
    for (const fin_index* p : s->parts) t += f(p);
    return t;
}
int64_t fin_pindex_n_nodes(const fin_pindex* s) { return set_sum(s, fin_index_n_nodes); }
int64_t fin_pindex_n_kmers(const fin_pindex* s) { return set_sum(s, fin_index_n_kmers); }
int64_t fin_pindex_total_len(const fin_pindex* s) { return set_sum(s, fin_index_total_len); }
int64_t fin_pindex_size_in_bytes(const fin_pindex* s) { return set_sum(s, fin_index_size_in_bytes); }
int64_t fin_pindex_replica_table_bytes(const fin_pindex* s) {
    if (!s) return -1;
    int64_t t = 0;
    for (const fin_index* p : s->parts) { const int64_t v = fin_index_replica_table_bytes(p, s->device); if (v > 0) t += v; }
    return t;
}
int fin_pindex_unitig_ids(const fin_pindex* s, uint32_t part, uint32_t* out, uint64_t n) {
    if (!s || part >= s->gid.size() || !out || n != s->gid[part].size()) return FIN_EINVAL;
    std::memcpy(out, s->gid[part].data(), n * sizeof(uint32_t));
    return FIN_OK;
}

// every part's replica on the set's device, and the parts' tables of set-wide unitig numbers
static int pindex_upload(fin_pindex* s, char* err, size_t errlen) {
    HIPCHK(hipSetDevice(s->device));
    for (size_t p = 0; p < s->parts.size(); p++) {
        const int rc = fin_index_to_device(s->parts[p], s->device, err, errlen);
        if (rc != FIN_OK) return rc;
        uint32_t* d = nullptr;
        if (hipMalloc(&d, s->gid[p].size() * sizeof(uint32_t) + 16) != hipSuccess) { (void)hipGetLastError(); set_err(err, errlen, "out of device memory (unitig numbers)"); return FIN_ENOMEM; }
        s->d_gid.push_back(d);
        HIPCHK(hipMemcpy(d, s->gid[p].data(), s->gid[p].size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    return FIN_OK;
}

// <prefix>.finparts (text: "finito-parts 1", k, the number of parts and unitigs, what the build's check counted, per part its first input unitig and its number of
// unitigs), <prefix>.p<i>.finamd (the part's container, fin_index_save) and <prefix>.p<i>.gid (its table of set-wide unitig numbers, u32 each)
int fin_pindex_save(const fin_pindex* s, const char* prefix, char* err, size_t errlen) {
    if (!s || !prefix) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    const std::string pre(prefix);
    PartsManifest old;   // (read before it is overwritten: the part files it names beyond this set's are removed below)
    (void)read_parts_manifest(pre, old);
    for (size_t p = 0; p < s->parts.size(); p++) {
        const std::string pp = pre + ".p" + std::to_string(p);
        const int rc = index_save_container(s->parts[p], pp.c_str(), err, errlen);
        if (rc != FIN_OK) return rc;
        FILE* f = fopen((pp + ".gid").c_str(), "wb");
        if (!f || fwrite(s->gid[p].data(), sizeof(uint32_t), s->gid[p].size(), f) != s->gid[p].size() || fclose(f) != 0) { set_err(err, errlen, "cannot write " + pp + ".gid"); if (f) fclose(f); return FIN_EIO; }
    }
    FILE* f = fopen((pre + ".finparts").c_str(), "w");
    if (!f) { set_err(err, errlen, "cannot write " + pre + ".finparts"); return FIN_EIO; }
    fprintf(f, "finito-parts 1\nk %d\nparts %zu\nunitigs %llu\nshared_kmers %lld\n", s->k, s->parts.size(), (unsigned long long)s->n_unitigs, (long long)s->shared_kmers);
    for (size_t p = 0; p < s->parts.size(); p++) fprintf(f, "part %zu first_unitig %llu unitigs %zu\n", p, (unsigned long long)s->first_unitig[p], s->gid[p].size());
    if (fclose(f) != 0) { set_err(err, errlen, "cannot write " + pre + ".finparts"); return FIN_EIO; }
    // what was under this prefix before is replaced: the higher-numbered parts of a larger set (no manifest names them any more), a one-index container
    if (const int rc = remove_part_files(pre, s->parts.size(), old.parts(), err, errlen)) return rc;
    return remove_file(pre + ".finamd", err, errlen);
}
int fin_pindex_exists(const char* prefix) { return prefix && file_exists(std::string(prefix) + ".finparts") ? 1 : 0; }
int fin_pindex_load(const char* prefix, int device, fin_pindex** out, char* err, size_t errlen) {
    if (!prefix || !out) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    const std::string pre(prefix);
    PartsManifest m;
    const int have = read_parts_manifest(pre, m);
    if (have < 0) { set_err(err, errlen, "cannot open " + pre + ".finparts"); return FIN_EIO; }
    if (have == 0) { set_err(err, errlen, pre + ".finparts is not a partitioned index's manifest"); return FIN_EIO; }
    std::unique_ptr<fin_pindex, void (*)(fin_pindex*)> s(new fin_pindex, fin_pindex_free);
    s->device = device; s->k = m.k;
    const size_t P = m.parts();
    const unsigned long long nu = m.n_unitigs;
    const std::vector<size_t>& cnt = m.n_part_unitigs;
    s->first_unitig = m.first_unitig; s->first_unitig.push_back(nu);
    s->n_unitigs = nu; s->shared_kmers = m.shared_kmers;
    uint64_t seen = 0;
    for (size_t p = 0; p < P; p++) {
        const std::string pp = pre + ".p" + std::to_string(p);
        fin_index* x = nullptr;
        const int rc = fin_index_load(pp.c_str(), &x, err, errlen);
        if (rc != FIN_OK) return rc;
        s->parts.push_back(x);
        if (fin_index_k(x) != s->k || (size_t)fin_index_n_unitigs(x) != cnt[p]) { set_err(err, errlen, pp + ".finamd does not belong to this manifest"); return FIN_EIO; }
        s->gid.emplace_back(cnt[p]);
        FILE* g = fopen((pp + ".gid").c_str(), "rb");
        const bool gok = g && fread(s->gid[p].data(), sizeof(uint32_t), cnt[p], g) == cnt[p];
        if (g) fclose(g);
        if (!gok) { set_err(err, errlen, "cannot read " + pp + ".gid"); return FIN_EIO; }
        for (uint32_t v : s->gid[p]) if (v >= nu) { set_err(err, errlen, pp + ".gid holds a unitig number beyond the set"); return FIN_EIO; }
        seen += cnt[p];
    }
    if (seen != nu) { set_err(err, errlen, pre + ".finparts: the parts' unitigs do not add up"); return FIN_EIO; }
    const int rc = pindex_upload(s.get(), err, errlen);
    if (rc != FIN_OK) return rc;
    *out = s.release();
    return FIN_OK;
}

// Where to cut the input unitigs [u0, u1), which together hold a k-mer twice (same strand: what fin_index_is_disjoint counts), so that the front piece does not:
// *cut = the first unitig that holds a k-mer of a unitig before it.  Host, plain strings: this runs for the rare part of an unchecked set that needs it.
static int pindex_split_point(const char* B, const uint64_t* O, uint64_t u0, uint64_t u1, int k, uint64_t* cut, char* err, size_t errlen) {
    if (O[u1] - O[u0] > (1ull << 26)) {
        set_err(err, errlen, "index set: a part of more than 2^26 bases holds a k-mer twice; it is not split here -- pass a smaller max_part_bases, or a disjoint set");
        return FIN_ELIMIT;
    }
    std::unordered_map<std::string, uint64_t> owner;   // k-mer -> the first unitig that holds it
    for (uint64_t u = u0; u < u1; u++) {
        const uint64_t len = O[u + 1] - O[u];
        for (uint64_t i = 0; i + (uint64_t)k <= len; i++) {
            std::string m(B + O[u] + i, (size_t)k);
            for (char& c : m) c &= (char)0xDF;
            const auto ins = owner.emplace(std::move(m), u);
            if (ins.second) continue;
            if (ins.first->second == u) {
                set_err(err, errlen, "index set: input unitig " + std::to_string(u) + " holds a k-mer twice by itself: no part can hold it and answer for what it reports");
                return FIN_EINVAL;
            }
            *cut = u;
            return FIN_OK;
        }
    }
    set_err(err, errlen, "index set: a part holds a k-mer twice, but no unitig of it repeats a k-mer of another (bases other than ACGT?): it cannot be split");
    return FIN_EINVAL;
}

int fin_pindex_build_device(const char* unitig_bases, const uint64_t* unitig_offsets, uint64_t n_unitigs, int k, int device, uint64_t max_part_bases,
                               int verify, fin_pindex** out, char* err, size_t errlen) {
    if (!unitig_bases || !unitig_offsets || !out || n_unitigs == 0 || k < 2 || k > 255) { set_err(err, errlen, "bad argument"); return FIN_EINVAL; }
    if (n_unitigs >= 0x7FFFFFFFull) { set_err(err, errlen, "more than 2^31-1 unitigs: a pair's unitig number is an int32"); return FIN_ELIMIT; }
    if (max_part_bases == 0) max_part_bases = 3200000000ull;   // (about 3.2e9 nodes: room below 2^32 for the dummy nodes)
    if (max_part_bases > 4100000000ull) max_part_bases = 4100000000ull;
    std::unique_ptr<fin_pindex, void (*)(fin_pindex*)> s(new fin_pindex, fin_pindex_free);
    s->k = k; s->device = device; s->n_unitigs = n_unitigs;
    // parts: consecutive input unitigs while they fit
    s->first_unitig.push_back(0);
    {
        uint64_t in_part = 0;
        for (uint64_t u = 0; u < n_unitigs; u++) {
            const uint64_t len = unitig_offsets[u + 1] - unitig_offsets[u];
            if (len < (uint64_t)k) { set_err(err, errlen, "a unitig is shorter than k"); return FIN_EINVAL; }
            if (len > max_part_bases) { set_err(err, errlen, "a unitig is longer than a part may be"); return FIN_ELIMIT; }
            if (in_part + len > max_part_bases) { s->first_unitig.push_back(u); in_part = 0; }
            in_part += len;
        }
        s->first_unitig.push_back(n_unitigs);
    }
    for (size_t p = 0; p + 1 < s->first_unitig.size();) {
        const uint64_t u0 = s->first_unitig[p], nu = s->first_unitig[p + 1] - u0;
        fin_index* x = nullptr;
        const int rc = fin_index_build_device(unitig_bases, unitig_offsets + u0, nu, k, device, &x, nullptr, err, errlen);
        if (rc != FIN_OK) return rc;
        // An UNCHECKED set must still be made of parts that are disjoint by themselves: an index that holds a k-mer twice answers as the reference does over
        // duplicated unitigs -- its walk can follow the wrong copy's text and name places that do not spell the k-mer (common.hh:61-67) --, and then nothing could
        // be said about what the set returns.  Such a part is cut in front of the first unitig that repeats a k-mer of the unitigs before it, and built again.
        if (!verify && !fin_index_is_disjoint(x)) {
            fin_index_free(x);
            uint64_t cut = 0;
            if (const int src = pindex_split_point(unitig_bases, unitig_offsets, u0, u0 + nu, k, &cut, err, errlen)) return src;
            s->first_unitig.insert(s->first_unitig.begin() + (ptrdiff_t)p + 1, cut);
            continue;   // ([u0, cut) holds no k-mer twice; [cut, ...) is looked at in its turn)
        }
        s->parts.push_back(x);
        p++;
    }
    const size_t P = s->first_unitig.size() - 1;
    // the set's unitig numbers: permute_unitigs over ALL unitigs -- colex order of the first k-mers (the last base is the most significant), ties by input order
    {
        std::vector<uint32_t> order(n_unitigs);
        for (uint64_t u = 0; u < n_unitigs; u++) order[u] = (uint32_t)u;
        auto code = [](char c) -> int { c &= (char)0xDF; return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3; };
        const char* const B = unitig_bases; const uint64_t* const O = unitig_offsets;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            const char* x = B + O[a], *y = B + O[b];
            for (int j = k - 1; j >= 0; j--) { const int cx = code(x[j]), cy = code(y[j]); if (cx != cy) return cx < cy; }
            return false;
        });
        // (walk the order once: a part's c-th unitig in it is that part's unitig number c)
        s->gid.assign(P, {});
        for (size_t p = 0; p < P; p++) s->gid[p].reserve(s->first_unitig[p + 1] - s->first_unitig[p]);
        for (uint64_t r = 0; r < n_unitigs; r++) {
            const uint64_t u = order[r];
            const size_t p = (size_t)(std::upper_bound(s->first_unitig.begin(), s->first_unitig.end(), u) - s->first_unitig.begin()) - 1;
            s->gid[p].push_back((uint32_t)r);
        }
    }
    // replicas and the number tables
    { const int rc = pindex_upload(s.get(), err, errlen); if (rc != FIN_OK) return rc; }
    if (verify) {
        const auto t0 = std::chrono::steady_clock::now();
        int64_t shared = 0;
        for (size_t p = 0; p < P; p++)
            if (!fin_index_is_disjoint(s->parts[p])) shared += fin_index_total_len(s->parts[p]) - (int64_t)(s->first_unitig[p + 1] - s->first_unitig[p]) * (k - 1) - fin_index_n_kmers(s->parts[p]);
        // a part's unitigs, as reads, in every part behind it (merged search: a k-mer or its reverse complement there is a hit)
        for (size_t p = 0; p + 1 < P && P > 1; p++) {
            for (size_t t = p + 1; t < P; t++) {
                fin_batch* b = nullptr;
                uint64_t u = s->first_unitig[p];
                const uint64_t u_end = s->first_unitig[p + 1];
                while (u < u_end) {
                    uint64_t v = u, bases = 0;
                    while (v < u_end && (v == u || bases + (unitig_offsets[v + 1] - unitig_offsets[v]) <= (1ull << 31)) && v - u < (1ull << 27)) { bases += unitig_offsets[v + 1] - unitig_offsets[v]; v++; }
                    int rc = b ? fin_batch_reload(b, unitig_bases, unitig_offsets + u, v - u, err, errlen)
                               : fin_batch_create_on(s->parts[t], device, unitig_bases, unitig_offsets + u, v - u, &b, err, errlen);
                    uint64_t npos = 0;
                    if (rc == FIN_OK) rc = fin_batch_run(b, FIN_MERGED, nullptr, err, errlen);
                    if (rc == FIN_OK) rc = fin_batch_download(b, nullptr, &npos, err, errlen);
                    if (rc != FIN_OK) { fin_batch_free(b); return rc; }
                    shared += (int64_t)npos;
                    u = v;
                }
                fin_batch_free(b);
            }
        }
        s->shared_kmers = shared;
        s->verify_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (shared != 0) {
            set_err(err, errlen, "index set: " + std::to_string(shared) + " k-mer occurrence(s) are not the only one of their k-mer (or of its reverse complement) in the set -- "
                                 "not a disjoint spectrum-preserving string set; parts cannot tell which occurrence the whole index would report");
            return FIN_EINVAL;
        }
    }
    *out = s.release();
    return FIN_OK;
}

struct fin_pbatch {
    const fin_pindex* set = nullptr;   // a reference (fin_pindex::refs): the set outlives the batch, whichever is freed first
    std::vector<fin_batch*> b;
    struct Ev { hipEvent_t e0, e1; };
    static constexpr size_t MAX_RUNS = 1024;   // the timing window: the event pairs of the most recent runs
    std::vector<Ev> runs;
    uint64_t runs_dropped = 0;         // runs whose events left the window: runs[i] is run number runs_dropped + i since creation
    hipStream_t last_stream = nullptr; bool ran = false;
};
void fin_pbatch_free(fin_pbatch* sb) {
    if (!sb) return;
    if (sb->set && sb->set->device >= 0) (void)hipSetDevice(sb->set->device);
    for (auto& r : sb->runs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    for (fin_batch* x : sb->b) fin_batch_free(x);   // (before the set's reference goes: they live on its parts)
    pindex_release(sb->set);
    delete sb;
}
int fin_pbatch_create(const fin_pindex* s, const char* bases, const uint64_t* offsets, uint64_t n_reads, fin_pbatch** out, char* err, size_t errlen) {
    if (!s || !out || !offsets) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    std::unique_ptr<fin_pbatch, void (*)(fin_pbatch*)> sb(new fin_pbatch, fin_pbatch_free);
    sb->set = s; s->refs.fetch_add(1, std::memory_order_relaxed);
    for (fin_index* p : s->parts) {
        fin_batch* x = nullptr;
        const int rc = fin_batch_create_on(p, s->device, bases, offsets, n_reads, &x, err, errlen);
        if (rc != FIN_OK) return rc;
        sb->b.push_back(x);
    }
    *out = sb.release();
    return FIN_OK;
}
int fin_pbatch_reload(fin_pbatch* sb, const char* bases, const uint64_t* offsets, uint64_t n_reads, char* err, size_t errlen) {
    if (!sb || !offsets) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    for (fin_batch* x : sb->b) { const int rc = fin_batch_reload(x, bases, offsets, n_reads, err, errlen); if (rc != FIN_OK) return rc; }
    sb->ran = false;
    return FIN_OK;
}
uint64_t fin_pbatch_n_kmers(const fin_pbatch* sb) { return (sb && !sb->b.empty()) ? sb->b[0]->n_kmers : 0; }
void* fin_pbatch_device_pairs(const fin_pbatch* sb) { return (sb && !sb->b.empty()) ? sb->b[0]->d_out : nullptr; }
// one step of the set: every part's step (fin_batch_run, merged strands) and its merge into the first part's output buffer, all on `hip_stream`
int fin_pbatch_run(fin_pbatch* sb, void* hip_stream, char* err, size_t errlen) {
    if (!sb || sb->b.empty()) { set_err(err, errlen, "bad argument"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(sb->set->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (sb->runs.size() >= fin_pbatch::MAX_RUNS) {
        (void)hipEventDestroy(sb->runs.front().e0); (void)hipEventDestroy(sb->runs.front().e1);
        sb->runs.erase(sb->runs.begin()); sb->runs_dropped++;
    }
    fin_pbatch::Ev ev;
    HIPCHK(hipEventCreate(&ev.e0)); HIPCHK(hipEventCreate(&ev.e1));
    sb->runs.push_back(ev);
    HIPCHK(hipEventRecord(ev.e0, st));
    for (size_t p = 0; p < sb->b.size(); p++) {
        const int rc = fin_batch_run(sb->b[p], FIN_MERGED, hip_stream, err, errlen);
        if (rc != FIN_OK) return rc;
        const int e = fin_launch_set_merge(sb->b[0]->d_out, sb->b[p]->d_out, sb->set->d_gid[p], sb->b[p]->n_kmers, p == 0 ? 1 : 0, st);
        if (e != 0) { set_err(err, errlen, std::string("merge kernel launch failed: ") + hipGetErrorString((hipError_t)e)); return FIN_ENODEV; }
    }
    HIPCHK(hipEventRecord(ev.e1, st));
    sb->last_stream = st; sb->ran = true;
    return FIN_OK;
}
int fin_pbatch_download(fin_pbatch* sb, int32_t* pairs_out, uint64_t* n_positive, char* err, size_t errlen) {
    if (!sb || sb->b.empty() || !sb->ran) { set_err(err, errlen, "fin_pbatch_download: nothing has run"); return FIN_EINVAL; }
    HIPCHK(hipSetDevice(sb->set->device));
    HIPCHK(hipStreamSynchronize(sb->last_stream));
    // (a part whose overflow list overran withholds its results: the set's are then incomplete)
    for (fin_batch* x : sb->b) { const int rc = batch_overrun_check(x, sb->last_stream, err, errlen); if (rc != FIN_OK) return rc; }
    fin_batch* b0 = sb->b[0];
    hipStream_t st = sb->last_stream;
    unsigned long long c = 0;
    if (n_positive && b0->n_kmers) {
        const int rc = fin_launch_count_positive(b0->d_out, b0->n_kmers, b0->d_count, st);
        if (rc != 0) { set_err(err, errlen, std::string("count kernel launch failed: ") + hipGetErrorString((hipError_t)rc)); return FIN_ENODEV; }
        HIPCHK(hipMemcpyAsync(&c, b0->d_count, 8, hipMemcpyDeviceToHost, st));
    }
    if (pairs_out && b0->n_kmers) HIPCHK(hipMemcpyAsync(pairs_out, b0->d_out, b0->n_kmers * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_positive) *n_positive = c;
    return FIN_OK;
}
// device time of a set step (HIP events on the launch stream), averaged over the runs behind the first skip_first SINCE CREATION that are still in the
// window (the skipped runs the window has dropped already count as skipped)
int fin_pbatch_step_time(const fin_pbatch* sb, uint64_t skip_first, double* ms_avg, uint64_t* n_runs) {
    if (!sb || !ms_avg) return FIN_EINVAL;
    double t = 0; uint64_t n = 0;
    const uint64_t from = skip_first > sb->runs_dropped ? skip_first - sb->runs_dropped : 0;
    for (size_t i = (size_t)std::min<uint64_t>(from, sb->runs.size()); i < sb->runs.size(); i++) {
        float ms = 0;
        if (hipEventSynchronize(sb->runs[i].e1) != hipSuccess || hipEventElapsedTime(&ms, sb->runs[i].e0, sb->runs[i].e1) != hipSuccess) { (void)hipGetLastError(); continue; }
        t += ms; n++;
    }
    *ms_avg = n ? t / (double)n : 0.0;
    if (n_runs) *n_runs = n;
    return FIN_OK;
}
// merged search of a flat read set in every part of the set (host buffers; one device batch per part)
int fin_pindex_search_batch(const fin_pindex* s, const char* bases, const uint64_t* offsets, uint64_t n_reads, int32_t* pairs_out, uint64_t* n_positive,
                               char* err, size_t errlen) {
    if (!s) { set_err(err, errlen, "null argument"); return FIN_EINVAL; }
    std::lock_guard<std::mutex> g(s->mu);   // (one search at a time per set: its parts share the device's memory with the cached batches)
    int rc = s->cached ? fin_pbatch_reload(s->cached, bases, offsets, n_reads, err, errlen) : fin_pbatch_create(s, bases, offsets, n_reads, &s->cached, err, errlen);
    if (rc == FIN_OK) rc = fin_pbatch_run(s->cached, nullptr, err, errlen);
    if (rc == FIN_OK) rc = fin_pbatch_download(s->cached, pairs_out, n_positive, err, errlen);
    if (rc != FIN_OK) { fin_pbatch_free(s->cached); s->cached = nullptr; }
    return rc;
}

}  // extern "C"
