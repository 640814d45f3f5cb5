// main.cpp -- the `finito` command: same sub-commands, flags, help/exit behaviour, log lines and output text as the
// reference's `benchmark` binary (src/main.cpp:21-59, include/build_fmin.hh:302-402, include/search_fmin.hh:130-213),
// with the search running on the MI355X through the C ABI.
//
// Differences, all on the build side: the reference reads a plain-matrix SBWT produced by the external `sbwt build`
// tool (-i) and takes k from it; here the SBWT is a pure function of the unitigs and k and is rebuilt, so -i is optional:
// when given, k is taken from the file and the file (and an --lcs file) must match what was rebuilt; without it k comes
// from -k (default 31).  --type rarest (-t 1) builds an index; --type shortest / verify print the reference's finimizer
// statistics for threshold -t (build_fmin.hh:252-268).  The index is one container file <prefix>.finamd; --sdsl 1 also writes
// the reference's seven files, and search-fmin -i <prefix> loads those when there is no container (fin_sdsl.cpp).
#include <omp.h>
#include <zlib.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <exception>
#include <fstream>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <iostream>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "FinimizerIndex.hh"

using namespace std;

static int64_t cur_time_micros() {
    return chrono::duration_cast<chrono::microseconds>(chrono::steady_clock::now().time_since_epoch()).count();
}
static void write_log(const string& msg) { cerr << msg << endl; }

// ---- FASTA / FASTQ reader, plain or gzipped (SBWT's SeqIO::Reader in the reference) ------------------------------
class SeqReader {
    gzFile f;
    vector<char> buf; size_t pos = 0, lim = 0;
    bool eof = false;
    int getc_() {
        if (pos == lim) {
            if (eof) return -1;
            int n = gzread(f, buf.data(), (unsigned)buf.size());
            if (n <= 0) { eof = true; return -1; }
            pos = 0; lim = (size_t)n;
        }
        return (unsigned char)buf[pos++];
    }
    int peek_() { int c = getc_(); if (c >= 0) pos--; return c; }
    void skip_line() {
        for (;;) {
            if (pos == lim && peek_() < 0) return;
            const char* nl = (const char*)memchr(buf.data() + pos, '\n', lim - pos);
            if (nl) { pos = (size_t)(nl - buf.data()) + 1; return; }
            pos = lim;
        }
    }
    void read_line(string& out) {
        for (;;) {
            if (pos == lim && peek_() < 0) return;
            const char* b = buf.data() + pos;
            const char* nl = (const char*)memchr(b, '\n', lim - pos);
            size_t n = nl ? (size_t)(nl - b) : lim - pos;
            size_t m = n;
            if (m && b[m - 1] == '\r') m--;
            out.append(b, m);
            pos += n + (nl ? 1 : 0);
            if (nl) return;
        }
    }

public:
    string read_buf;
    explicit SeqReader(const string& path) : buf(1 << 20) {
        f = gzopen(path.c_str(), "rb");
        if (!f) throw runtime_error("Error opening file " + path);
    }
    ~SeqReader() { if (f) gzclose(f); }
    // returns the length of the next sequence, 0 at end of file (get_next_read_to_buffer of the reference)
    int64_t get_next_read_to_buffer() {
        read_buf.clear();
        int c;
        while ((c = peek_()) >= 0 && (c == '\n' || c == '\r')) getc_();
        if (c < 0) return 0;
        if (c == '>') {
            skip_line();
            while ((c = peek_()) >= 0 && c != '>') read_line(read_buf);
        } else if (c == '@') {
            skip_line();
            read_line(read_buf);
            skip_line();   // '+'
            skip_line();   // qualities (multi-line FASTQ is not supported, as in the reference)
        } else {
            throw runtime_error("Error: input is neither FASTA nor FASTQ");
        }
        return (int64_t)read_buf.size();
    }
};

// ---- a team of host threads that SLEEP between jobs ---------------------------------------------------------------------------
// The stages of search-fmin work side by side, each with all host threads.  OpenMP teams would spin at the end of every parallel
// region (libgomp's default wait policy, fixed when the runtime loads): under a container's CPU quota the idle spinning of three
// teams gets every stage throttled (measured on a 16-core share: parser 3.1 s instead of 0.2 s).  These threads wait on a
// condition variable instead.
class Team {
    vector<thread> th; mutex mu; condition_variable cv, done_cv;
    const function<void(int, int)>* job = nullptr; uint64_t gen = 0; int pending = 0; bool quit = false;
    void worker(int t) {
        uint64_t seen = 0;
        for (;;) {
            const function<void(int, int)>* j;
            { unique_lock<mutex> g(mu); cv.wait(g, [&] { return quit || gen != seen; }); if (quit) return; seen = gen; j = job; }
            (*j)(t, n);
            { lock_guard<mutex> g(mu); if (--pending == 0) done_cv.notify_one(); }
        }
    }
public:
    const int n;
    explicit Team(int n_) : n(n_ < 1 ? 1 : n_) { for (int t = 1; t < n; t++) th.emplace_back([this, t] { worker(t); }); }
    ~Team() { { lock_guard<mutex> g(mu); quit = true; } cv.notify_all(); for (auto& t : th) t.join(); }
    // f(t, n) on every member t of the team; returns when all are done.  An exception in a member is rethrown here.
    void run(const function<void(int, int)>& f) {
        exception_ptr err; mutex emu;
        const function<void(int, int)> safe = [&](int t, int nn) { try { f(t, nn); } catch (...) { lock_guard<mutex> g(emu); if (!err) err = current_exception(); } };
        { lock_guard<mutex> g(mu); job = &safe; pending = n - 1; gen++; }
        cv.notify_all();
        safe(0, n);
        { unique_lock<mutex> g(mu); done_cv.wait(g, [&] { return pending == 0; }); }
        if (err) rethrow_exception(err);
    }
    // [lo, hi) of member t when N items are dealt out evenly
    static pair<size_t, size_t> share(size_t N, int t, int n) { return {N * (size_t)t / (size_t)n, N * (size_t)(t + 1) / (size_t)n}; }
};

// ---- block-parallel reader for uncompressed files (f-3: the reference parses one read at a time, search_fmin.hh:43-45) -----------
// The file is read in blocks of a few hundred MB; in a block all threads look for line starts, then for records (FASTQ: groups of
// four lines, checked for their '@' and '+'; FASTA: from one '>' line to the next, sequence lines concatenated), then copy the
// sequences side by side into the caller's buffer.  A block that does not look regular (blank lines inside a FASTQ, a stray
// character) is parsed by the sequential rules of SeqReader instead, so both readers accept the same files and give the same reads.
class BlockReader {
    int fd = -1;
    const char* map = nullptr; size_t size = 0, pos = 0;   // the file, mapped; everything before pos has been parsed
    vector<vector<uint32_t>> nl; vector<uint32_t> ends;    // (kept between blocks: no allocation per block)
    Team team{fin_host_threads()};
    static bool is_gzip(const string& path) {
        unsigned char m[2] = {0, 0};
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) throw runtime_error("Error opening file " + path);
        const size_t n = fread(m, 1, 2, f); fclose(f);
        return n == 2 && m[0] == 0x1f && m[1] == 0x8b;
    }
    // the sequential rules (SeqReader::get_next_read_to_buffer) over memory; returns bytes consumed (whole records only unless `last`)
    static size_t parse_sequential(const char* p, size_t n, bool last, char* dst, size_t& n_bases, vector<uint64_t>& offsets) {
        size_t i = 0, done = 0;
        auto line_end = [&](size_t from) -> size_t { const char* nl = (const char*)memchr(p + from, '\n', n - from); return nl ? (size_t)(nl - p) : n; };
        for (;;) {
            while (i < n && (p[i] == '\n' || p[i] == '\r')) i++;
            if (i >= n) { done = n; break; }
            const size_t rec = i;
            if (p[i] == '>') {
                size_t e = line_end(i); if (e == n && !last) { done = rec; break; }
                i = e + 1;
                const size_t b0 = n_bases;
                bool complete = false;
                for (;;) {
                    if (i >= n) { complete = last; break; }
                    if (p[i] == '>') { complete = true; break; }
                    e = line_end(i);
                    if (e == n && !last) break;
                    size_t m = e - i; if (m && p[i + m - 1] == '\r') m--;
                    memcpy(dst + n_bases, p + i, m); n_bases += m;
                    i = e + 1;
                }
                if (!complete) { n_bases = b0; done = rec; break; }
                if (n_bases > b0) offsets.push_back(n_bases);   // (an empty sequence ends the reference's loop, search_fmin.hh:44; here it is skipped)
                done = i < n ? i : n;
            } else if (p[i] == '@') {
                // header, sequence, '+', qualities; at the end of the file a truncated record still yields its sequence line
                size_t ls[4] = {0, 0, 0, 0}, le[4] = {0, 0, 0, 0}; size_t j = i; int got = 0;
                for (int l = 0; l < 4 && j <= n; l++) {
                    ls[l] = j; le[l] = j < n ? line_end(j) : n;
                    const bool has_nl = le[l] < n;
                    if (!has_nl && !last) break;   // an incomplete line: wait for more data
                    got++;
                    j = le[l] + 1;
                    if (!has_nl) break;            // the file's last line, without '\n'
                }
                if (got < 4 && !last) { done = rec; break; }
                if (got >= 2) {
                    size_t m = le[1] - ls[1]; if (m && p[ls[1] + m - 1] == '\r') m--;
                    if (m) { memcpy(dst + n_bases, p + ls[1], m); n_bases += m; offsets.push_back(n_bases); }
                }
                if (got < 4 || le[3] >= n) { done = n; break; }
                i = le[3] + 1;
                done = i;
            } else throw runtime_error("Error: input is neither FASTA nor FASTQ");
        }
        return done;
    }

public:
    // a regular, uncompressed file that can be mapped
    static bool usable(const string& path) {
        if (is_gzip(path)) return false;
        struct stat st;
        return stat(path.c_str(), &st) == 0 && S_ISREG(st.st_mode);
    }
    explicit BlockReader(const string& path) {
        fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) throw runtime_error("Error opening file " + path);
        struct stat st;
        if (fstat(fd, &st) != 0) throw runtime_error("Error opening file " + path);
        size = (size_t)st.st_size;
        if (size) {
            void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) throw runtime_error("Error mapping file " + path);
            map = (const char*)m;
            (void)madvise(m, size, MADV_SEQUENTIAL);
        }
    }
    ~BlockReader() { if (map) munmap((void*)map, size); if (fd >= 0) close(fd); }
    // Next block of reads: bases side by side into dst (room for `block_bytes` bases), offsets = {0, end of read 0, ...}.
    // Returns false at the end of the file.  dst_grow(n) must return a buffer of at least n bytes, keeping nothing.
    template <class Grow>
    bool next(size_t block_bytes, Grow dst_grow, size_t& n_bases, vector<uint64_t>& offsets) {
        n_bases = 0; offsets.assign(1, 0);
        size_t want = block_bytes;
        for (;;) {
            if (pos >= size) return false;
            const size_t n = min(want, size - pos);
            const bool eof = pos + n == size;
            char* dst = dst_grow(n);
            const char* p = map + pos;
            size_t consumed = 0;
            // ---- line starts, all threads ----
            const int nt = team.n;
            if (nl.size() < (size_t)nt) nl.resize((size_t)nt);
            for (auto& v : nl) v.clear();
            bool regular = n < 0xFFFFFFF0ull;
            if (regular) {
                team.run([&](int t, int tn) {
                    const size_t lo = n * (size_t)t / (size_t)tn, hi = n * (size_t)(t + 1) / (size_t)tn;
                    vector<uint32_t>& v = nl[(size_t)t];
                    for (const char* q = p + lo; q < p + hi;) {
                        const char* x = (const char*)memchr(q, '\n', (size_t)(p + hi - q));
                        if (!x) break;
                        v.push_back((uint32_t)(x - p)); q = x + 1;
                    }
                });
            }
            vector<size_t> base((size_t)nt + 1, 0);
            for (int t = 0; t < nt; t++) base[(size_t)t + 1] = base[(size_t)t] + nl[(size_t)t].size();
            const size_t n_nl = base[(size_t)nt];
            if (ends.size() < n_nl) ends.resize(n_nl + n_nl / 8);   // position of every '\n'
            team.run([&](int t, int) { if (!nl[(size_t)t].empty()) memcpy(ends.data() + base[(size_t)t], nl[(size_t)t].data(), nl[(size_t)t].size() * 4); });
            auto line_start = [&](size_t l) -> size_t { return l == 0 ? 0 : (size_t)ends[l - 1] + 1; };
            const size_t n_lines = n_nl + ((eof && (n_nl == 0 ? n > 0 : (size_t)ends[n_nl - 1] + 1 < n)) ? 1 : 0);   // a last line without '\n' counts at the end of the file
            auto line_len = [&](size_t l) -> size_t {
                const size_t s0 = line_start(l), e = l < n_nl ? (size_t)ends[l] : n;
                size_t m = e - s0; if (m && p[s0 + m - 1] == '\r') m--;
                return m;
            };
            bool parsed = false;
            if (regular && n_lines >= 1 && p[0] == '@') {
                // FASTQ: groups of four lines (before the end of the file only lines that end in '\n' count)
                const size_t full = n_lines / 4, rem = n_lines % 4;
                const size_t n_rec = full + ((eof && rem >= 2) ? 1 : 0);   // a truncated last record still has its sequence line
                bool ok = n_rec > 0;
                {
                    vector<char> okt((size_t)nt, 1);
                    team.run([&](int t, int tn) {
                        const auto sh = Team::share(full, t, tn);
                        bool o = true;
                        for (size_t r = sh.first; r < sh.second && o; r++) o = p[line_start(4 * r)] == '@' && p[line_start(4 * r + 2)] == '+' && line_len(4 * r + 1) > 0;
                        okt[(size_t)t] = o;
                    });
                    for (char o : okt) ok = ok && o;
                }
                if (ok && n_rec > full) ok = p[line_start(4 * full)] == '@' && line_len(4 * full + 1) > 0;
                if (ok) {
                    offsets.resize(n_rec + 1);
                    team.run([&](int t, int tn) { const auto sh = Team::share(n_rec, t, tn); for (size_t r = sh.first; r < sh.second; r++) offsets[r + 1] = line_len(4 * r + 1); });
                    for (size_t r = 0; r < n_rec; r++) offsets[r + 1] += offsets[r];
                    team.run([&](int t, int tn) {
                        const auto sh = Team::share(n_rec, t, tn);
                        for (size_t r = sh.first; r < sh.second; r++) memcpy(dst + offsets[r], p + line_start(4 * r + 1), (size_t)(offsets[r + 1] - offsets[r]));
                    });
                    n_bases = (size_t)offsets[n_rec];
                    consumed = eof ? n : line_start(4 * full);
                    parsed = true;
                }
            } else if (regular && n_lines >= 1 && p[0] == '>') {
                // FASTA: a record runs from its '>' line to the next one
                vector<vector<uint32_t>> hd((size_t)nt);
                team.run([&](int t, int tn) {
                    const auto sh = Team::share(n_lines, t, tn);
                    for (size_t l = sh.first; l < sh.second; l++) { const size_t s0 = line_start(l); if (s0 < n && p[s0] == '>') hd[(size_t)t].push_back((uint32_t)l); }
                });
                vector<uint32_t> heads;
                for (auto& v : hd) heads.insert(heads.end(), v.begin(), v.end());
                const size_t n_rec = eof ? heads.size() : (heads.empty() ? 0 : heads.size() - 1);   // the last record may go on in the next block
                if (n_rec > 0) {
                    vector<uint64_t> len(n_rec + 1, 0);
                    // (records are dealt out by their first line, so that members get about the same number of lines whatever the record sizes)
                    auto rec_share = [&](int t, int tn) -> pair<size_t, size_t> {
                        const auto ls = Team::share(n_lines, t, tn);
                        const size_t a = (size_t)(lower_bound(heads.begin(), heads.begin() + (long)n_rec, (uint32_t)ls.first) - heads.begin());
                        const size_t b = t + 1 == tn ? n_rec : (size_t)(lower_bound(heads.begin(), heads.begin() + (long)n_rec, (uint32_t)ls.second) - heads.begin());
                        return {a, b};
                    };
                    team.run([&](int t, int tn) {
                        const auto sh = rec_share(t, tn);
                        for (size_t r = sh.first; r < sh.second; r++) {
                            const size_t l1 = r + 1 < heads.size() ? heads[r + 1] : n_lines;
                            uint64_t m = 0;
                            for (size_t l = (size_t)heads[r] + 1; l < l1; l++) m += line_len(l);
                            len[r + 1] = m;
                        }
                    });
                    for (size_t r = 0; r < n_rec; r++) len[r + 1] += len[r];
                    team.run([&](int t, int tn) {
                        const auto sh = rec_share(t, tn);
                        for (size_t r = sh.first; r < sh.second; r++) {
                            const size_t l1 = r + 1 < heads.size() ? heads[r + 1] : n_lines;
                            char* d = dst + len[r];
                            for (size_t l = (size_t)heads[r] + 1; l < l1; l++) { const size_t m = line_len(l); memcpy(d, p + line_start(l), m); d += m; }
                        }
                    });
                    // reads without bases are skipped, as by the sequential rules
                    offsets.assign(1, 0);
                    bool any_empty = false;
                    for (size_t r = 0; r < n_rec; r++) any_empty |= len[r + 1] == len[r];
                    if (!any_empty) { offsets.resize(n_rec + 1); for (size_t r = 0; r <= n_rec; r++) offsets[r] = len[r]; }
                    else for (size_t r = 0; r < n_rec; r++) if (len[r + 1] > len[r]) offsets.push_back(len[r + 1]);
                    n_bases = (size_t)len[n_rec];
                    consumed = eof ? n : line_start(heads[n_rec]);
                    parsed = true;
                }
            }
            if (!parsed) consumed = parse_sequential(p, n, eof, dst, n_bases, offsets);
            pos += consumed;
            if (offsets.size() > 1) return true;
            if (eof) return false;                       // nothing but blank lines / an unfinished tail was left
            want = want + (want >> 1) + block_bytes / 4; // no complete record yet (one record larger than the block): look further
        }
    }
};

static vector<string> readlines(const string& path) {
    ifstream in(path);
    if (!in.good()) throw runtime_error("Error opening file " + path);
    vector<string> v; string line;
    while (getline(in, line)) if (!line.empty()) v.push_back(line);
    return v;
}
static void check_readable(const string& path) {
    ifstream in(path);
    if (!in.good()) throw runtime_error("Error reading file: " + path);
}
static void check_writable(const string& path) {
    ofstream out(path, ios::app);
    if (!out.good()) throw runtime_error("Error writing to file: " + path);
}

// ---- tiny option parser with cxxopts' surface for the flags the two commands use --------------------------------
struct Opts {
    map<string, string> val; bool help = false;
    bool has(const string& k) const { return val.count(k) > 0; }
    string get(const string& k, const string& def = "") const { auto it = val.find(k); return it == val.end() ? def : it->second; }
};
static Opts parse(int argc, char** argv, const map<string, string>& short_to_long, const vector<string>& longs) {
    Opts o;
    for (int i = 1; i < argc; i++) {
        string a = argv[i], key, value; bool have_value = false;
        if (a == "-h" || a == "--help") { o.help = true; continue; }
        if (a.rfind("--", 0) == 0) {
            key = a.substr(2);
            size_t eq = key.find('=');
            if (eq != string::npos) { value = key.substr(eq + 1); key = key.substr(0, eq); have_value = true; }
        } else if (a.size() >= 2 && a[0] == '-') {
            string s = a.substr(1, 1);
            auto it = short_to_long.find(s);
            if (it == short_to_long.end()) throw runtime_error("Option '" + a + "' does not exist");
            key = it->second;
            if (a.size() > 2) { value = a.substr(2); have_value = true; }
        } else throw runtime_error("Unexpected argument: " + a);
        bool known = false;
        for (auto& l : longs) known |= l == key;
        if (!known) throw runtime_error("Option '" + a + "' does not exist");
        if (!have_value) {
            if (i + 1 >= argc) throw runtime_error("Option '" + a + "' is missing an argument");
            value = argv[++i];
        }
        o.val[key] = value;
    }
    return o;
}

static const char* BUILD_HELP =
    "Find all Finimizers of all input reads.\nUsage:\n  build-fmin [OPTION...]\n\n"
    "  -o, --out-file arg    Output index filename prefix.\n"
    "  -i, --index-file arg  SBWT file of the unitigs (plain-matrix, from `sbwt build`). Optional here: the SBWT is rebuilt\n"
    "                        from the unitigs; when given, k is taken from it and it is checked against the rebuilt one.\n"
    "  -u, --in-file arg     The SPSS in FASTA or FASTQ format, possibly gzipped. Multi-line FASTQ is not\n"
    "                        supported. If the file extension is .txt, this is interpreted as a list of\n"
    "                        files, one per line.\n"
    "  -k arg                k-mer length when no SBWT file is given (default: 31)\n"
    "      --type arg        Decide which streaming search type you prefer. Available types:  rarest shortest verify. The latter two only provide some stats. (default: rarest)\n"
    "  -t arg                Maximum finimizer frequency (default: 1)\n"
    "      --lcs arg         LCS file of the SBWT; checked against the recomputed LCS. (default: \"\")\n"
    "      --sdsl arg        1: also write the reference's own index files <prefix>.*.sdsl + <prefix>.sbwt\n"
    "      --parts-max-bases N  build a PARTITIONED index: parts of at most N bases of unitigs, each an ordinary index (automatic above 4e9 bases:\n"
    "                          one index holds fewer than 2^32 nodes); needs a GPU and a disjoint spectrum-preserving string set\n"
    "      --device-build arg  0: build on the host; 1: build on the GPU or fail; default: GPU when there is one\n"
    "      --device arg      HIP device ordinal of the device build (default: 0)\n"
    "      --threads arg     Host threads for construction (default: all)\n"
    "  -h, --help            Print usage\n";

static const char* SEARCH_HELP =
    "Query all Finimizers of all input reads.\nUsage:\n  search-fmin [OPTION...]\n\n"
    "  -o, --out-file arg    Output filename, or stdout if not given.\n"
    "  -i, --index-file arg  Index filename prefix.\n"
    "  -q, --query-file arg  The query in FASTA or FASTQ format, possibly gzipped. Multi-line FASTQ is not\n"
    "                        supported. If the file extension is .txt, this is interpreted as a list of\n"
    "                        query files, one per line. In this case, --out-file is also interpreted as a\n"
    "                        list of output files in the same manner, one line for each input file.\n"
    "      --device arg      first HIP device ordinal (default: 0)\n"
    "      --gpus arg        number of GPUs to shard the reads over, index replicated (default: all visible)\n"
    "      --strand-counts arg  1: also count the k-mers found on each strand by itself, as the reference logs them (\"Found kmers\",\n"
    "                        \"Found kmers reverse\") and sums them into <index>.stats: two more search passes per read (default: 0 --\n"
    "                        the stats field is then the merged count)\n"
    "      --unitig-counts FILE  also write the run's profile over the unitig set: one line `unitig<TAB>count` per unitig of the index, in\n"
    "                        unitig order, zeros included -- how many query k-mers (both strands merged, all query files) were found in it.\n"
    "                        Counted on the first GPU, nothing per k-mer comes back for it. Not for a partitioned index.\n"
    "      --unitig-coverage FILE  also write the run's breadth over the unitig set: one line `unitig<TAB>kmers<TAB>covered` per unitig of the\n"
    "                        index, in unitig order -- kmers = length - k + 1, covered = how many DISTINCT k-mers of the unitig were found (a\n"
    "                        bitmap on the first GPU, one bit per base of the unitig text). Goes with --unitig-counts. Not for a partitioned index.\n"
    "                        Costs one more search of every chunk on the device, beside the one for the text and the one for\n"
    "                        --unitig-counts; with --no-text 1 and no --unitig-counts a chunk is still searched twice (the second\n"
    "                        pass counts the found k-mers the log reports).\n"
    "      --unitig-depth FILE  also write the run's per-position depth over the unitig set, summed up per unitig: one line\n"
    "                        `unitig<TAB>kmers<TAB>sum<TAB>max<TAB>solid` per unitig of the index, in unitig order -- kmers = length - k + 1, sum = the\n"
    "                        unitig's count of --unitig-counts, max = the most often any one of its k-mers was found, solid = how many of its k-mers\n"
    "                        were found at least T times (--min-depth). Kept on the first GPU, 4 bytes per base of the unitig text, from one more\n"
    "                        search of every chunk; goes with -o, --unitig-counts, --unitig-coverage and --segments. Not for a partitioned index.\n"
    "      --min-depth T     the T of --unitig-depth and --color-coverage (default: 1); only with one of them\n"
    "      --pileup FILE     also write the run's base pileup over the unitig text: a line unitig<TAB>offset<TAB>ref<TAB>cover<TAB>A<TAB>C<TAB>G<TAB>T\n"
    "                        for every position a placed read spans (cover > 0) -- how many reads span it and how many show each base other\n"
    "                        than the text's -- and a last line #reads<TAB>kept<TAB>not_straight<TAB>off_unitig<TAB>too_many. A read is placed when\n"
    "                        its found k-mers lie on one diagonal of one unitig and the whole read lies inside it. Kept on the first GPU, 20 bytes\n"
    "                        per base of the unitig text, from one more pass over each chunk. Not for a partitioned index.\n"
    "      --variants FILE   the same columns for the candidate positions only, called on the GPU: the greatest alt count is at least\n"
    "                        --min-alt N (default: 2) and at least --min-alt-permille P thousandths of the cover (default: 200)\n"
    "      --pileup-max-mismatch M  reads with more than M mismatches are left out of the pileup (0 .. 255, default: 8)\n"
    "      --segments FILE   also write every read's path through the unitig set: one line `read<TAB>slot<TAB>length<TAB>unitig<TAB>offset<TAB>+|-` per\n"
    "                        segment -- `length` consecutive k-mers of read `read` (0-based ordinal in the query file, counted through a list of\n"
    "                        query files), from its k-mer number `slot` on, found in `unitig` at `offset`, `offset + 1`, ... (+) or `offset`,\n"
    "                        `offset - 1`, ... (-). Reads without a found k-mer have no line. Made on the first GPU from one more search of every\n"
    "                        chunk; goes with -o, --unitig-counts and --unitig-coverage. Not for a partitioned index.\n"
    "      --read-summary FILE  also write one line per read, in input order: `read<TAB>k-mers<TAB>found<TAB>segments<TAB>longest<TAB>span` -- `read` as\n"
    "                        --segments prints it, k-mers = length - k + 1 (0 for a shorter read), found = how many of them were found, segments = the\n"
    "                        read's number of --segments lines, longest = the longest of them, span = last found k-mer - first found k-mer + 1.\n"
    "                        Made on the first GPU from one more search of every chunk, 16 bytes per read come back; goes with -o, --unitig-counts,\n"
    "                        --unitig-coverage, --unitig-depth, --segments and --screen. Not for a partitioned index.\n"
    "      --screen FILE     also write the numbers of the reads that pass the screen, one per line, ascending: a read passes when found >= N and\n"
    "                        1000 * found >= P * k-mers (found, k-mers as in --read-summary). Decided on the first GPU from one more search of every\n"
    "                        chunk, one bit per read comes back; goes with everything --read-summary goes with. Not for a partitioned index. The reads\n"
    "                        themselves are not written. With --no-text 1 and no --unitig-counts, --segments or --read-summary a chunk is searched\n"
    "                        twice (the second pass counts the found k-mers the log reports).\n"
    "      --min-found N     the N of --screen (default: 1)\n"
    "      --min-permille P  the P of --screen, 0 to 1000 (default: 0)\n"
    "      --screen-invert arg  1: write the reads that do NOT pass (default: 0)\n"
    "      --label-unitigs FASTA  the unitigs the index was built from, in the order --labels speaks of (needed by --classify and --label-report)\n"
    "      --labels FILE     one line per record of --label-unitigs, in its order: the unitig's label, a non-negative integer, or `-` for none (k-mers\n"
    "                        found in such a unitig vote for no label)\n"
    "      --classify FILE   also write one line per read, in input order: `read<TAB>k-mers<TAB>label<TAB>best<TAB>second<TAB>labelled` -- `read` and k-mers\n"
    "                        as in --read-summary, label = the label most of the read's found k-mers carry (ties: the smaller one; `-` if none is labelled),\n"
    "                        best = how many carry it, second = how many carry the runner-up, labelled = how many carry any label. Made on the first GPU\n"
    "                        from one more search of every chunk, 16 bytes per read come back; goes with everything --read-summary goes with. Not for a\n"
    "                        partitioned index.\n"
    "      --label-report FILE  also write `label<TAB>reads` per label, then `unassigned<TAB>reads`: a read is assigned to its label when best >= max(N, 1),\n"
    "                        1000 * best >= P * k-mers and best >= second + M. Tallied on the first GPU from one more search of every chunk, nothing per\n"
    "                        read comes back; goes with everything --read-summary goes with. Not for a partitioned index.\n"
    "      --class-min-found N     the N of --label-report (default: 1)\n"
    "      --class-min-permille P  the P of --label-report, 0 to 1000 (default: 0)\n"
    "      --class-min-margin M    the M of --label-report (default: 0; 1 leaves ties unassigned)\n"
    "      --color-refs LIST  colour the index's unitigs by search: LIST holds one FASTA/FASTQ path per line, the line's number (from 0, empty lines\n"
    "                        skipped, at most 4096) is the colour; every sequence of file c is searched on the first GPU and every unitig in which one of\n"
    "                        its k-mers is found gets colour c. Sequences longer than 4096 k-mers are cut into windows that overlap by k - 1 bases, so\n"
    "                        that no k-mer is lost. Needed by --colors-out and --pseudoalign. Not for a partitioned index.\n"
    "      --colors-out FILE  write `unitig<TAB>c1,c2,...` per unitig of the index, in the index's unitig numbers, `-` for a unitig without a colour\n"
    "      --color-coverage FILE  also write the run's breadth and depth per reference of --color-refs: one line\n"
    "                        `colour<TAB>kmers<TAB>covered<TAB>kmers_only<TAB>covered_only<TAB>depth_sum<TAB>depth_sum_only<TAB>solid<TAB>solid_only` per colour --\n"
    "                        the k-mers of the unitigs that carry the colour, how many of them were found, their summed depth and how many were found at\n"
    "                        least T times (--min-depth), and the same over the unitigs that carry this colour alone --, then a line\n"
    "                        `uncoloured<TAB>kmers<TAB>covered<TAB>depth_sum<TAB>solid` over the unitigs without a colour. Projected on the first GPU after the\n"
    "                        last chunk from a coverage bitmap and a depth kept there (those of --unitig-coverage / --unitig-depth when they are asked for\n"
    "                        too), at their cost: one more search of every chunk each. Coverage counts k-mers, so with --paired 1 mates need no pairing.\n"
    "                        Wants --color-refs; goes with --no-text 1, --abundance, --eqclasses, --assign-weights and --paired 1. Not for a partitioned index.\n"
    "      --depth-histogram FILE  also write the run's k-mer spectrum, binned on the GPU after the last chunk: one line depth<TAB>k-mers per bin -- how many\n"
    "                        k-mer positions of the unitig text were found that many times; the last bin's depth is written >=X. Bins: --depth-bins B (1 .. 1024,\n"
    "                        default 256) of --depth-bin-width D depths each (default 1), bin(d) = min(d / D, B - 1). Goes with -o and every per-unitig output.\n"
    "      --color-depth-histogram FILE  with --color-refs: the same per reference. Lines colour<TAB>all|only<TAB>depth<TAB>k-mers for the non-zero entries (all: over\n"
    "                        the unitigs that carry the colour, only: over those that carry it alone), then uncoloured<TAB>-<TAB>depth<TAB>k-mers.\n"
    "      --color-depth-quantiles FILE  with --color-refs: the quartiles of every reference's k-mer depth, read from those histograms. Lines\n"
    "                        colour<TAB>kmers<TAB>q250<TAB>q500<TAB>q750<TAB>kmers_only<TAB>q250_only<TAB>q500_only<TAB>q750_only; - where there are no\n"
    "                        k-mers, >=X where the quantile lies in the last bin. Neither colour file goes with --compact-colors 1.\n"
    "      --compact-colors 1  with --color-refs: after the colouring and before the first chunk of reads, deduplicate the colour rows on the GPU\n"
    "                        (every distinct colour set once and a set id per unitig instead of the dense matrix). Prints\n"
    "                        'colour sets<TAB>n_sets<TAB>bytes dense<TAB>bytes compact' to stderr; every per-read and per-run colour output is byte-identical.\n"
    "                        Not with --color-coverage, --color-similarity or --taxonomy (they read the dense matrix).\n"
    "      --color-sets-out PREFIX  with --compact-colors 1: PREFIX.set_of.u32 (uint32 per unitig) and PREFIX.sets.u64 (W uint64 per set, set 0 empty), raw little-endian.\n"
    "      --color-similarity FILE  also write what the references of --color-refs share, integers only: one line\n"
    "                        `colour_a<TAB>colour_b<TAB>size_a<TAB>size_b<TAB>shared` per pair a < b with shared > 0, ascending -- the k-mers of the unitigs that\n"
    "                        carry a, that carry b, and that carry both --, then one line `identical<TAB>c1,c2,...` per group of references with the same\n"
    "                        column of the colour matrix (no estimate can tell its members apart). The colour matrix times itself on the first GPU, right\n"
    "                        after the colouring. Wants --color-refs; goes with everything --color-coverage goes with.\n"
    "      --color-similarity-covered FILE2  the same over the k-mers the run found: sizes and shared count found k-mers only. Made after the last chunk\n"
    "                        from a coverage bitmap kept on the first GPU (that of --unitig-coverage / --color-coverage when they are asked for too), at its\n"
    "                        cost: one more search of every chunk. Wants --color-similarity.\n"
    "      --pseudoalign FILE  also write one line per read, in input order: `read<TAB>k-mers<TAB>found<TAB>coloured<TAB>c1,c2,...` -- `read` and k-mers as\n"
    "                        in --read-summary, found = the k-mers found, coloured = those of them in a unitig with a colour, then the colours that at\n"
    "                        least P thousandths of the coloured k-mers have (`-` for none). Made on the first GPU from one more search of every chunk;\n"
    "                        goes with everything --read-summary goes with. Not for a partitioned index.\n"
    "      --pseudo-permille P  the P of --pseudoalign, --eqclasses and --color-report, 0 to 1000 (default: 1000, the intersection; 0 is the union)\n"
    "      --taxonomy FILE   a tree over taxa: one line `id<TAB>parent_id` per taxon, any integer ids (NCBI's, say), the root its own parent. A cycle, an\n"
    "                        unknown parent, a second root and a repeated id are errors that name the line. Wants --color-taxa and --taxa or --taxon-report.\n"
    "      --color-taxa FILE  one taxon id per line, the taxon of the reference on the same line of --color-refs (empty lines do not count). A unitig's taxon is\n"
    "                        the lowest common ancestor of its references' taxa, made on the GPU after the colouring.\n"
    "      --taxa FILE       also write one line per read, in input order: `read<TAB>k-mers<TAB>taxon<TAB>score<TAB>clade<TAB>labelled` -- the deepest taxon\n"
    "                        the read's k-mers support (Kraken's root-to-leaf rule; `-`: unclassified), the best root-to-leaf score, the k-mers at or below\n"
    "                        the taxon and the k-mers that have a taxon at all. Made on the GPU; goes with -o and the other per-run outputs, and with --no-text 1.\n"
    "      --taxon-report FILE  also write `taxon<TAB>clade_reads<TAB>direct_reads` for every taxon with a read at or below it, then `unclassified<TAB>N`.\n"
    "      --taxa-confidence P  a call moves up the tree until its clade holds P thousandths of the read's k-mers, 0 to 1000 (default: 0)\n"
    "      --taxa-min-found N   ... and at least N k-mers (default: 1). Not for a partitioned index, not with --paired 1.\n"
    "      --eqclasses FILE  the equivalence classes of the reads under the colours of --color-refs: one line `reads<TAB>n_colours<TAB>c1,c2,...` per\n"
    "                        distinct non-empty colour set a read has at the P of --pseudo-permille, reads = how many reads have it, in ascending order\n"
    "                        of the sets as bit rows. Accumulated on the first GPU from one more search of every chunk, nothing per read comes back;\n"
    "                        written after the last chunk. Goes with everything --read-summary goes with. Not for a partitioned index.\n"
    "      --color-report FILE  from the same classes: `colour<TAB>reads<TAB>reads_only` for every colour -- the reads whose set contains the colour and\n"
    "                        the reads whose set is that colour alone --, then `unaligned<TAB>N`, the reads without a colour\n"
    "      --eq-max-classes N  room for N distinct colour sets, 1 to 67108864 (default: 1048576); more is an error\n"
    "      --eqclasses-in LIST  a file with one path per line, each a classes file as --eqclasses writes it (optionally ended by `unaligned<TAB>N`), made\n"
    "                        under the same --color-refs: their classes are added on the GPU before the first chunk, exactly and in integers, so\n"
    "                        --eqclasses, --color-report and --abundance (with --ab-bootstraps) cover the earlier runs and this one. A colour at or above\n"
    "                        the number of references, a malformed line or a wrong n_colours is an error that names file and line. Only legal together\n"
    "                        with --eqclasses, --color-report or --abundance\n"
    "      --eqclasses-unaligned 1  end the file of --eqclasses with the line `unaligned<TAB>N`, the reads without a colour, so that --eqclasses-in carries\n"
    "                        them into a later run (default: no such line). Only legal together with --eqclasses\n"
    "      --abundance FILE  from the same classes, on the GPU: expected reads per reference by EM (each class's reads split over its colours in\n"
    "                        proportion to the current estimate, repeated). `colour<TAB>reads<TAB>share` per colour -- reads = the expected reads, share =\n"
    "                        reads / length over its sum, both as %.10g --, then `unaligned<TAB>N`, `iterations<TAB>T<TAB>converged` (or `max_iters`) and\n"
    "                        `loglik<TAB>L`. Goes with --eqclasses and --color-report (one accumulator for all three) and with --no-text 1.\n"
    "      --ab-lengths FILE  one positive number per line, line number = colour: the effective length of each reference (default: all 1).\n"
    "                        Empty lines are skipped and do not count, as in the list of --color-refs\n"
    "      --ab-max-iters N  at most N iterations, 1 to 100000 (default: 1000)\n"
    "      --ab-tol X        stop once no colour's reads change by more than X max(reads, 1) (default: 1e-6)\n"
    "      --ab-bootstraps B  with --abundance: B bootstrap replicates of the estimate, 1 to 4096, the class counts of each resampled on the GPU (a Poisson\n"
    "                        bootstrap keyed by the class's colour set: the same reads and seed give the same replicates). Every colour line gains\n"
    "                        `<TAB>boot_mean<TAB>boot_sd` -- mean and standard deviation (B - 1 in the divisor; 0 for B = 1) of the replicates' reads, as %.10g --,\n"
    "                        and a line `bootstraps<TAB>B<TAB>seed<TAB>S` follows the `loglik` line\n"
    "      --ab-seed S       the seed of --ab-bootstraps, an unsigned 64-bit number (default: 0)\n"
    "      --assign-weights FILE  assign every read (with --paired 1: every fragment) to references, on the GPU, from per-reference weights: FILE is what\n"
    "                        --abundance wrote in an earlier run over the same --color-refs, its `reads` column divided by the lengths of --ab-lengths where\n"
    "                        given (lines `unaligned`, `iterations`, `loglik`, `bootstraps` and bootstrap columns are ignored). Colour c of a read's colour set\n"
    "                        at --pseudo-permille is assigned iff weight[c] > 0 and weight[c] >= threshold[c] * (the sum of the set's weights).\n"
    "                        Wants --color-refs and --assign and / or --assign-report; goes with --no-text 1, --pseudoalign, --eqclasses and --abundance.\n"
    "      --assign-threshold X  X: one number from 0 to 1 for every colour (default: 0.5); `abundance`: the `share` column of the weights file\n"
    "      --assign FILE     one line per read or fragment, in input order: `read<TAB>best<TAB>c1,c2,...` -- best = the colour of its set with the largest\n"
    "                        weight, then the assigned colours; `-` where there is none\n"
    "      --assign-report FILE  `colour<TAB>assigned<TAB>sole` per colour (reads the colour is assigned to; reads assigned to it alone), then\n"
    "                        `unaligned<TAB>N`, `unassigned<TAB>N` (a colour set, none assigned) and `multi<TAB>N` (two or more assigned)\n"
    "      --paired arg      1: the query file holds INTERLEAVED mates, records 2f and 2f + 1 are fragment f (needs --color-refs). Chunks are cut after an\n"
    "                        even number of records; a file with an odd number of records is an error. --pseudoalign then writes one line per fragment,\n"
    "                        `fragment<TAB>k-mers<TAB>found<TAB>coloured<TAB>coloured_first<TAB>c1,c2,...` -- the k-mers of both mates together, coloured_first = the\n"
    "                        first mate's share of coloured --, and --eqclasses, --color-report and --abundance count fragments: the definition of\n"
    "                        --pseudoalign over both mates' k-mers together (at P = 1000 the intersection of the mates' sets where both have coloured\n"
    "                        k-mers). Everything else is per read as before\n"
    "      --pair-both arg   1 (only with --paired 1): a fragment has colours only if BOTH mates have a coloured k-mer\n"
    "      --fragments FILE  with --paired 1: the geometry of every fragment, made on the GPU. Lines fragment<TAB>class<TAB>unitig<TAB>start<TAB>length<TAB>dir1<TAB>dir2;\n"
    "                        class 0 none, 1 one, 2 split, 3 tandem, 4 outward, 5 inward; dir F or R per placed mate; `-` where there is nothing to report\n"
    "      --fragment-lengths FILE  with --paired 1: the insert-size histogram of the inward fragments, written after the last chunk: length<TAB>fragments per\n"
    "                        non-zero bin (the last bin as >=X), the six class lines and mean<TAB>M. --fragment-bins B (1 .. 4096, default 1024) and\n"
    "                        --fragment-bin-width D (default 1): bin(len) = min(len / D, B - 1)\n"
    "      --ab-fragment-lengths arg  1 (with --paired 1, --abundance and --ab-lengths): the numbers of --ab-lengths are the references' lengths in bases; they\n"
    "                        become effective lengths under the run's own fragment-length histogram (bin width 1) after the last chunk, before the EM, and are\n"
    "                        written as a further column of the abundance file\n"
    "      --ref-paths LIST  reference coordinates: LIST names one FASTA/FASTQ file per line; every record is searched before the first chunk of reads and its\n"
    "                        path through the unitig set stays on the first GPU. Wants --ref-depth or --ref-variants; independent of --color-refs. Not for a\n"
    "                        partitioned index.\n"
    "      --ref-depth FILE  with --ref-paths: the depth of the run along every record, in windows of --ref-window W slots (1 .. 2147483648, default 1000),\n"
    "                        lifted on the GPU after the last chunk: ref<TAB>record<TAB>start<TAB>end<TAB>in_graph<TAB>covered<TAB>depth_sum, ref the line of LIST from 0,\n"
    "                        record the record's number in its file, [start, end) 0-based k-mer slots; covered counts against --min-depth\n"
    "      --ref-variants FILE  with --ref-paths: the pileup's candidates (--min-alt, --min-alt-permille, --pileup-max-mismatch) under every record that\n"
    "                        crosses them: ref<TAB>record<TAB>pos<TAB>+|-<TAB>ref_base<TAB>cover<TAB>A<TAB>C<TAB>G<TAB>T<TAB>unitig<TAB>offset, pos 1-based, bases and counts\n"
    "                        in the record's orientation\n"
    "      --links FILE      also write the junctions the reads crossed, counted on the GPU (include/finito_amd.h: LINKS): after the last chunk one line\n"
    "                        unitig_a<TAB>offset_a<TAB>unitig_b<TAB>offset_b<TAB>count per link, ascending by place, the a end the lower place; then\n"
    "                        #transitions<TAB>T, #links<TAB>D (distinct links), #self<TAB>S. Goes with -o, --no-text 1 and the per-unitig outputs.\n"
    "                        Not for a partitioned index.\n"
    "      --max-links N     the most distinct links the table of --links holds (default: 1048576; 1 to 268435456); the run fails beyond it\n"
    "      --links-min-count C  write only the links crossed at least C times (default: 1)\n"
    "      --no-text arg     1 (only with --unitig-counts, --unitig-coverage, --unitig-depth, --segments, --read-summary, --screen, --classify,\n"
    "                        --label-report, --colors-out, --pseudoalign, --eqclasses, --color-report or --abundance): do not make or write the pair\n"
    "                        text, the other results asked for are the only ones\n"
    "  -h, --help            Print usage\n";

static int build_fmin(int argc, char** argv) {
    Opts o = parse(argc, argv, {{"o", "out-file"}, {"i", "index-file"}, {"u", "in-file"}, {"t", "t"}, {"k", "k"}},
                   {"out-file", "index-file", "in-file", "type", "t", "lcs", "k", "threads", "sdsl", "device-build", "device", "parts-max-bases"});
    if (argc == 1 || o.help) { cerr << BUILD_HELP << endl; exit(1); }
    if (!o.has("in-file")) throw runtime_error("Option 'in-file' has no value");
    if (!o.has("out-file")) throw runtime_error("Option 'out-file' has no value");
    int64_t t = stoll(o.get("t", "1"));
    string type = o.get("type", "rarest");
    if (type != "rarest" && type != "shortest" && type != "verify") {   // build_fmin.hh:363-367
        cerr << "Error: unknown type: " << type << endl << "Available types are: rarest shortest verify" << endl; return 1;
    }
    if (type == "rarest" && t != 1) throw runtime_error("t != 1 does not make sense with rarest type");   // build_fmin.hh:245-247
    if (t < 1) throw runtime_error("t must be at least 1");
    // k: the reference takes it from the SBWT file given with -i (build_fmin.hh:363-364).  Here the SBWT is rebuilt from the unitigs, so
    // -i is optional; when it is given, k comes from it (a -k that disagrees is an error) and the file is checked against what was built.
    int k = stoi(o.get("k", "31"));
    const string sbwt_file = o.get("index-file"), lcs_file = o.get("lcs");
    if (!sbwt_file.empty()) {
        int64_t kf = 0, nn = 0, nk = 0; char err[512] = {0};
        if (fin_sbwt_file_info(sbwt_file.c_str(), &kf, &nn, &nk, err, sizeof err) != FIN_OK) throw runtime_error(string("Error loading index from file: ") + err);
        if (o.has("k") && (int64_t)k != kf) throw runtime_error("-k " + to_string(k) + " does not match the SBWT file (k = " + to_string(kf) + ")");
        k = (int)kf;
        write_log("Loading the index variant plain-matrix");
    }
    string in_file = o.get("in-file");
    vector<string> input_files;
    if (in_file.size() >= 4 && in_file.substr(in_file.size() - 4) == ".txt") input_files = readlines(in_file);
    else input_files = {in_file};
    for (auto& f : input_files) check_readable(f);
    string out_prefix = o.get("out-file");

    string bases; vector<uint64_t> offsets{0};
    for (auto& f : input_files) {
        write_log("Searching Finimizers from input file " + f + " to index prefix " + out_prefix);
        SeqReader reader(f);
        while (reader.get_next_read_to_buffer() > 0) { bases += reader.read_buf; offsets.push_back(bases.size()); }
    }
    FinimizerIndex index;
    // A unitig set beyond one index's 2^32 nodes (or --parts-max-bases N): a PARTITIONED index -- parts of at most N bases, each an ordinary index built and kept
    // on the GPU; search-fmin finds it by its manifest <prefix>.finparts.  Needs a GPU; the set must be what the reference requires, a disjoint spectrum-
    // preserving string set (README.md:79-80), which the build checks; only type rarest.
    const uint64_t parts_max = o.has("parts-max-bases") ? stoull(o.get("parts-max-bases")) : 0;
    if (parts_max || bases.size() >= 4000000000ull) {
        if (type != "rarest") throw runtime_error("a partitioned index (more than 4e9 bases of unitigs, or --parts-max-bases) is built for type rarest only");
        if (!sbwt_file.empty() || !lcs_file.empty()) throw runtime_error("-i / --lcs cannot be checked against a partitioned index");
        index.build_partitioned(bases, offsets, k, stoi(o.get("device", "0")), parts_max);
        write_log("Partitioned index built on the GPU: " + to_string(index.number_of_parts()) + " parts");
        write_log("#SBWT nodes: " + to_string(index.number_of_subsets()));
        write_log("#Distinct finimizers: " + to_string(index.number_of_finimizers()));
        index.serialize(out_prefix);
        ofstream pstats(out_prefix + "_stats.txt", ios::app);   // build_fmin.hh:386-399
        if (pstats.is_open()) {
            pstats << to_string(t) + "," << index.number_of_finimizers() << "," << index.number_of_finimizers() << ",1.000000,," << index.number_of_kmers() << "\n";
            cout << "String appended to the file successfully." << endl;
        } else cerr << "Error: Unable to open file." << endl;
        return 0;
    }
    // the device builder when there is a GPU and k <= 64 (the same index, bit for bit, about 30 times sooner: fin_build_gpu.hip), unless
    // --device-build 0; else the host builder
    const string want_dev = o.get("device-build", "auto");
    bool on_device = false;
    if (want_dev != "0" && want_dev != "false" && fin_device_count() > 0) {
        try { index.build_on_device(bases, offsets, k, stoi(o.get("device", "0"))); on_device = true; }
        catch (const exception& e) { if (want_dev != "auto") throw; write_log(string("device build failed (") + e.what() + "), using the host builder"); }
    }
    if (!on_device) index.build(bases, offsets, k, stoi(o.get("threads", "0")));
    write_log(on_device ? "Index built on the GPU" : "Index built on the host");
    if (!sbwt_file.empty() || !lcs_file.empty()) {   // -i / --lcs: must be the SBWT / LCS of these unitigs
        char err[512] = {0};
        if (fin_index_check_against_files(index.handle(), sbwt_file.c_str(), lcs_file.c_str(), err, sizeof err) != FIN_OK) throw runtime_error(err);
        if (!lcs_file.empty()) cerr << "LCS_file loaded" << endl;
    }
    if (type != "rarest") {
        // statistics only, no index is written (build_fmin.hh:252-268); the log and the stats line are print_finimizer_stats' (common.hh:188-206)
        int64_t nf = 0, sum_freq = 0, sum_len = 0;
        index.finimizer_stats(bases, offsets, type == "shortest" ? FIN_STATS_SHORTEST : FIN_STATS_VERIFY, t, nf, sum_freq, sum_len);
        const string result = to_string(nf) + "," + to_string(sum_freq) + "," + to_string((float)sum_freq / (float)nf) + "," +
                              to_string((float)sum_len / (float)nf) + "," + to_string(index.number_of_kmers());
        write_log(to_string(t) + "," + result);
        write_log("#SBWT nodes: " + to_string(index.number_of_subsets()));
        write_log("#Distinct finimizers: " + to_string(nf));
        write_log("Sum of frequencies: " + to_string(sum_freq));
        write_log("Avg frequency: " + to_string((float)sum_freq / (float)nf));
        write_log("Avg length: " + to_string((float)sum_len / (float)nf));
        ofstream stats(out_prefix + "_stats.txt", ios::app);   // build_fmin.hh:386-399
        if (stats.is_open()) { stats << to_string(t) + "," << result << "\n"; cout << "String appended to the file successfully." << endl; }
        else cerr << "Error: Unable to open file." << endl;
        return 0;
    }
    write_log("#SBWT nodes: " + to_string(index.number_of_subsets()));
    write_log("#Distinct finimizers: " + to_string(index.number_of_finimizers()));
    index.serialize(out_prefix);
    if (o.has("sdsl") && o.get("sdsl") != "0" && o.get("sdsl") != "false") index.serialize_reference_layout(out_prefix);   // + the reference's own seven files (FinimizerIndex.hh:187-207)
    ofstream stats(out_prefix + "_stats.txt", ios::app);   // build_fmin.hh:386-399
    if (stats.is_open()) {
        stats << to_string(t) + "," << index.number_of_finimizers() << "," << index.number_of_finimizers() << ",1.000000,,"
              << index.number_of_kmers() << "\n";
        cout << "String appended to the file successfully." << endl;
    } else cerr << "Error: Unable to open file." << endl;
    return 0;
}

// ---- the streaming query loop (search_fmin.hh:33-84) as a three-stage host pipeline ------------------------------------
// parse (one thread) -> search (GPU, fin_search_batch on page-locked buffers) -> format + write (all host threads), chunks of
// ~256 MB of bases cycling through the stages, so the file parser, the PCIe/GPU work and the text formatter overlap.
struct PinnedBuf {   // page-locked host memory that only grows
    void* p = nullptr; size_t cap = 0;
    char* get(size_t n) {
        if (n > cap) {
            fin_host_free(p); p = nullptr; cap = 0;
            const size_t want = n + n / 8 + 4096;
            p = fin_host_alloc(want);
            if (!p) throw runtime_error("page-locked host allocation failed (no HIP device?)");
            cap = want;
        }
        return (char*)p;
    }
    ~PinnedBuf() { fin_host_free(p); }
};
// page-locked buffers made ready while the index loads (page-locking costs about 0.15 s per GB): the chunks of the first file pick
// them up instead of allocating in the pipeline
struct Prewarmed { vector<fin_text*> texts; vector<pair<void*, size_t>> bases; mutex mu; } g_prewarmed;
struct Chunk {
    PinnedBuf bases, pairs;
    fin_text* text = nullptr; bool as_text = false;   // the chunk's output text when the GPU formatted it
    ~Chunk() { fin_text_free(text); }
    size_t n_bases = 0;
    vector<uint64_t> offsets, pair_off;
    uint64_t positive = 0, positive_fwd = 0, positive_rev = 0;   // merged; --strand-counts: search(read) / search(rc(read)) each by itself
    vector<char> rc;                                             // --strand-counts: the chunk's reads reverse-complemented
    bool failed = false;
};
template <class T>
class BlockingQueue {
    mutex mu; condition_variable cv; deque<T> q;
public:
    void push(T v) { { lock_guard<mutex> g(mu); q.push_back(v); } cv.notify_one(); }
    T pop() { unique_lock<mutex> g(mu); cv.wait(g, [&] { return !q.empty(); }); T v = q.front(); q.pop_front(); return v; }
};
struct OutSink {   // regular files are written by all threads at once, anything else sequentially
    int fd = 1; bool seekable = false; uint64_t pos = 0; bool own = false;
    explicit OutSink(const string* path) {
        if (path) {
            fd = open(path->c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
            if (fd < 0) throw runtime_error("Error writing to file: " + *path);
            own = true;
        }
        struct stat st;
        seekable = fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && own;
    }
    ~OutSink() { if (own) close(fd); }
    static void write_all(int fd, const char* p, size_t n, int64_t at) {
        while (n) {
            ssize_t w = at >= 0 ? pwrite(fd, p, n, (off_t)at) : write(fd, p, n);
            if (w < 0) { if (errno == EINTR) continue; throw runtime_error(string("write failed: ") + strerror(errno)); }
            p += w; n -= (size_t)w; if (at >= 0) at += w;
        }
    }
};

// --strand-counts 1: kmers_count / kmers_count_rev of search_fmin.hh:66-67 -- the hits of search(read) and of search(rc(read)) each by
// itself, which the merged pairs do not show (a forward hit hides the reverse strand's) -- from two forward-only passes per chunk
static bool g_strand_counts = false;
// --unitig-counts FILE: every chunk's hits are added into one accumulator on the first device (fin_search_batch_add_hits), downloaded once after the last
// chunk; --no-text 1: that is all a chunk is searched for
static fin_hits* g_hits = nullptr;   // (with --no-text 1 there is one even without --unitig-counts: its sum is the run's found k-mers)
// --unitig-coverage FILE: the same for the coverage bitmap (fin_search_batch_add_cover)
static fin_cover* g_cover = nullptr;
static void add_cover_chunk(const FinimizerIndex& index, const char* bases, const uint64_t* offsets, uint64_t n_reads) {
    char err[512] = {0};
    if (fin_search_batch_add_cover(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_cover, err, sizeof err) != FIN_OK) throw runtime_error(err);
}
// --unitig-depth FILE: the same for the per-position depth (fin_search_batch_add_depth)
static fin_depth* g_depth = nullptr;
static void add_depth_chunk(const FinimizerIndex& index, const char* bases, const uint64_t* offsets, uint64_t n_reads) {
    char err[512] = {0};
    if (fin_search_batch_add_depth(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_depth, err, sizeof err) != FIN_OK) throw runtime_error(err);
}
// --links FILE: the same for the junctions the reads cross (fin_search_batch_add_links)
static fin_links* g_links = nullptr;
static void add_links_chunk(const FinimizerIndex& index, const char* bases, const uint64_t* offsets, uint64_t n_reads) {
    char err[512] = {0};
    if (fin_search_batch_add_links(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_links, err, sizeof err) != FIN_OK) throw runtime_error(err);
}
// --pileup FILE / --variants FILE: the same for the base pileup (fin_search_batch_add_pileup)
static fin_pileup* g_pileup = nullptr;
static fin_refpaths* g_refpaths = nullptr;   // --ref-paths: the references' paths through the unitig set, made before the first chunk
static void add_pileup_chunk(const FinimizerIndex& index, const char* bases, const uint64_t* offsets, uint64_t n_reads) {
    char err[512] = {0};
    if (fin_search_batch_add_pileup(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_pileup, err, sizeof err) != FIN_OK) throw runtime_error(err);
}
// --segments FILE: every chunk's segments are made on the first device (fin_search_batch_segments) and written as lines, by the search stage, in chunk order
static FILE* g_seg_file = nullptr;
static uint64_t g_seg_read0 = 0;   // reads in the chunks (and query files) before this one
static double g_seg_per_read = 0;   // the most segments per read a chunk has had
static vector<uint64_t> g_seg_offs; static vector<fin_segment> g_segs; static string g_seg_text;
static uint64_t segments_chunk(const FinimizerIndex& index, const char* bases, const uint64_t* offsets, uint64_t n_reads, uint64_t n_kmers) {
    char err[512] = {0};
    // room for four segments per read at first (a read is rarely more than two or three), or half as many again as the densest chunk so far needed; a chunk
    // that needs more says how many and is searched once more with exactly that room -- one per k-mer always suffices
    g_seg_offs.resize(n_reads + 1);
    uint64_t n_seg = 0, pos = 0, cap = min<uint64_t>(n_kmers, (uint64_t)(max(4.0, 1.5 * g_seg_per_read) * (double)n_reads) + 1024);
    for (;;) {
        if (g_segs.size() < cap + 1) g_segs.resize(cap + 1);
        const int rc = fin_search_batch_segments(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_seg_offs.data(), g_segs.data(), cap, &n_seg, &pos, err, sizeof err);
        if (rc == FIN_OK) break;
        if (rc != FIN_ELIMIT || n_seg <= cap) throw runtime_error(err);
        cap = n_seg;
    }
    if (n_reads) g_seg_per_read = max(g_seg_per_read, (double)n_seg / (double)n_reads);
    string& t = g_seg_text;
    t.clear();
    for (uint64_t r = 0; r < n_reads; r++)
        for (uint64_t q = g_seg_offs[r]; q < g_seg_offs[r + 1]; q++) {
            const fin_segment& S = g_segs[q];
            t += to_string(g_seg_read0 + r); t += '\t'; t += to_string(S.slot); t += '\t'; t += to_string(S.len < 0 ? -(int64_t)S.len : (int64_t)S.len); t += '\t';
            t += to_string(S.u); t += '\t'; t += to_string(S.off); t += S.len < 0 ? "\t-\n" : "\t+\n";
        }
    if (!t.empty() && fwrite(t.data(), 1, t.size(), g_seg_file) != t.size()) throw runtime_error("Error writing the segments file");
    g_seg_read0 += n_reads;
    return pos;
}
// --read-summary FILE: every chunk's per-read summaries are made on the first device (fin_search_batch_read_summaries) and written as lines, by the search
// stage, in chunk order.  --screen FILE: the same for the screen (fin_search_batch_screen): the passing reads' run-wide numbers
static FILE* g_rs_file = nullptr;
static uint64_t g_rs_read0 = 0;   // reads in the chunks (and query files) before this one
static vector<fin_read_summary> g_rs; static string g_rs_text;
static uint64_t read_summary_chunk(const FinimizerIndex& index, const char* bases, const uint64_t* offsets, uint64_t n_reads, const uint64_t* pair_off) {
    char err[512] = {0};
    g_rs.resize(n_reads + 1);
    uint64_t pos = 0;
    if (fin_search_batch_read_summaries(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_rs.data(), &pos, err, sizeof err) != FIN_OK) throw runtime_error(err);
    string& t = g_rs_text;
    t.clear();
    for (uint64_t r = 0; r < n_reads; r++) {
        const fin_read_summary& S = g_rs[r];
        t += to_string(g_rs_read0 + r); t += '\t'; t += to_string(pair_off[r + 1] - pair_off[r]); t += '\t'; t += to_string(S.n_found); t += '\t';
        t += to_string(S.n_segments); t += '\t'; t += to_string(S.longest); t += '\t'; t += to_string(S.span); t += '\n';
    }
    if (!t.empty() && fwrite(t.data(), 1, t.size(), g_rs_file) != t.size()) throw runtime_error("Error writing the read summary file");
    g_rs_read0 += n_reads;
    return pos;
}
static FILE* g_scr_file = nullptr;
static uint64_t g_scr_read0 = 0;
static uint32_t g_scr_min_found = 1, g_scr_min_permille = 0; static int g_scr_invert = 0;
static vector<uint64_t> g_scr_bits; static string g_scr_text;
static void screen_chunk(const FinimizerIndex& index, const char* bases, const uint64_t* offsets, uint64_t n_reads) {
    char err[512] = {0};
    g_scr_bits.assign((n_reads + 63) / 64 + 1, 0);
    if (fin_search_batch_screen(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_scr_min_found, g_scr_min_permille, g_scr_invert, g_scr_bits.data(), nullptr, err, sizeof err) != FIN_OK)
        throw runtime_error(err);
    string& t = g_scr_text;
    t.clear();
    for (uint64_t w = 0; w < (n_reads + 63) / 64; w++)
        for (uint64_t x = g_scr_bits[w]; x; x &= x - 1) { t += to_string(g_scr_read0 + 64 * w + (uint64_t)__builtin_ctzll(x)); t += '\n'; }
    if (!t.empty() && fwrite(t.data(), 1, t.size(), g_scr_file) != t.size()) throw runtime_error("Error writing the screen file");
    g_scr_read0 += n_reads;
}
// --classify FILE: every chunk's per-read classes under the labelling of --label-unitigs / --labels are made on the first device (fin_search_batch_classify) and
// written as lines, by the search stage, in chunk order.  --label-report FILE: every chunk's reads are tallied on the device (fin_search_batch_add_classes)
static fin_labels* g_labels = nullptr;
static FILE* g_cls_file = nullptr;
static bool g_cls_report = false;
static uint64_t g_cls_read0 = 0;
static uint32_t g_cls_min_found = 1, g_cls_min_permille = 0, g_cls_min_margin = 0;
static vector<fin_read_class> g_cls; static string g_cls_text;
static void classify_chunk(const FinimizerIndex& index, const char* bases, const uint64_t* offsets, uint64_t n_reads, const uint64_t* pair_off) {
    char err[512] = {0};
    if (g_cls_file) {
        g_cls.resize(n_reads + 1);
        if (fin_search_batch_classify(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_labels, g_cls.data(), nullptr, err, sizeof err) != FIN_OK) throw runtime_error(err);
        string& t = g_cls_text;
        t.clear();
        for (uint64_t r = 0; r < n_reads; r++) {
            const fin_read_class& S = g_cls[r];
            t += to_string(g_cls_read0 + r); t += '\t'; t += to_string(pair_off[r + 1] - pair_off[r]); t += '\t';
            if (S.label == FIN_NO_LABEL) t += '-'; else t += to_string(S.label);
            t += '\t'; t += to_string(S.n_best); t += '\t'; t += to_string(S.n_second); t += '\t'; t += to_string(S.n_labelled); t += '\n';
        }
        if (!t.empty() && fwrite(t.data(), 1, t.size(), g_cls_file) != t.size()) throw runtime_error("Error writing the classification file");
    }
    if (g_cls_report && fin_search_batch_add_classes(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_labels, g_cls_min_found, g_cls_min_permille, g_cls_min_margin,
                                                     err, sizeof err) != FIN_OK)
        throw runtime_error(err);
    g_cls_read0 += n_reads;
}
// --taxa FILE: every chunk's reads are called by Kraken's rule under the taxonomy of --taxonomy / --color-taxa on the first device (fin_search_batch_taxa) and
// written as lines, taxa in the caller's ids.  --taxon-report FILE: every chunk's reads are tallied on the device (fin_search_batch_add_taxa)
static fin_taxonomy* g_tax = nullptr;
static FILE* g_tax_file = nullptr;
static bool g_tax_report = false;
static uint64_t g_tax_read0 = 0;
static uint32_t g_tax_min_found = 1, g_tax_confidence = 0;
static vector<int64_t> g_tax_ids;   // the caller's id of every taxon, by its number
static vector<fin_read_taxon> g_tax_reads; static string g_tax_text;
static void taxa_chunk(const FinimizerIndex& index, const char* bases, const uint64_t* offsets, uint64_t n_reads, const uint64_t* pair_off) {
    char err[512] = {0};
    if (g_tax_file) {
        g_tax_reads.resize(n_reads + 1);
        if (fin_search_batch_taxa(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_tax, g_tax_min_found, g_tax_confidence, g_tax_reads.data(), nullptr, err, sizeof err) != FIN_OK)
            throw runtime_error(err);
        string& t = g_tax_text;
        t.clear();
        for (uint64_t r = 0; r < n_reads; r++) {
            const fin_read_taxon& S = g_tax_reads[r];
            t += to_string(g_tax_read0 + r); t += '\t'; t += to_string(pair_off[r + 1] - pair_off[r]); t += '\t';
            if (S.taxon == FIN_NO_LABEL) t += '-'; else t += to_string(g_tax_ids[S.taxon]);
            t += '\t'; t += to_string(S.score); t += '\t'; t += to_string(S.clade); t += '\t'; t += to_string(S.n_labelled); t += '\n';
        }
        if (!t.empty() && fwrite(t.data(), 1, t.size(), g_tax_file) != t.size()) throw runtime_error("Error writing the taxa file");
    }
    if (g_tax_report && fin_search_batch_add_taxa(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_tax, g_tax_min_found, g_tax_confidence, err, sizeof err) != FIN_OK)
        throw runtime_error(err);
    g_tax_read0 += n_reads;
}
// one integer of a taxonomy file's line; false for anything else
static bool taxon_id(const string& v, int64_t& out) {
    size_t used = 0;
    try { out = stoll(v, &used); } catch (...) { return false; }
    return !v.empty() && used == v.size();
}
// --taxonomy FILE: `id<TAB>parent_id` per line, any integer ids, the root its own parent; empty lines are skipped (and still count as lines).  ids[t] = the id of
// taxon t in the topological numbering the library takes (the root 0, then breadth-first, siblings in file order), parent[t] in those numbers.  Every refusal
// names the line
static void taxonomy_parse_file(const string& path, vector<int64_t>& ids, vector<uint32_t>& parent, unordered_map<int64_t, uint32_t>& number) {
    ifstream in(path);
    if (!in) throw runtime_error("--taxonomy: cannot read " + path);
    auto bad = [&](size_t line, const string& what) { return runtime_error("--taxonomy: " + path + " line " + to_string(line) + ": " + what); };
    vector<int64_t> id, pid; vector<size_t> line_of;
    unordered_map<int64_t, size_t> at;
    string line;
    for (size_t n = 1; getline(in, line); n++) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const size_t tab = line.find('\t');
        int64_t a = 0, b = 0;
        if (tab == string::npos || !taxon_id(line.substr(0, tab), a) || !taxon_id(line.substr(tab + 1), b)) throw bad(n, "wants `id<TAB>parent_id`, two integers");
        if (at.count(a)) throw bad(n, "taxon " + to_string(a) + " was given on line " + to_string(line_of[at[a]]) + " already");
        at[a] = id.size(); id.push_back(a); pid.push_back(b); line_of.push_back(n);
    }
    if (id.empty()) throw runtime_error("--taxonomy: " + path + " is empty, it names no taxon");
    if (id.size() > 0x80000000ull) throw runtime_error("--taxonomy: " + path + " names more than 2^31 taxa");
    vector<vector<uint32_t>> kids(id.size());
    size_t root = id.size();
    for (size_t i = 0; i < id.size(); i++) {
        if (pid[i] == id[i]) {
            if (root != id.size()) throw bad(line_of[i], "a second root: taxon " + to_string(id[i]) + " is its own parent, as taxon " + to_string(id[root]) + " of line " + to_string(line_of[root]) + " is");
            root = i;
        } else {
            auto it = at.find(pid[i]);
            if (it == at.end()) throw bad(line_of[i], "taxon " + to_string(id[i]) + " has the unknown parent " + to_string(pid[i]));
            kids[it->second].push_back((uint32_t)i);
        }
    }
    if (root == id.size()) throw bad(line_of[0], "no root: no taxon is its own parent (every taxon lies on a cycle or below one)");
    vector<uint32_t> order{(uint32_t)root}, num(id.size(), 0xFFFFFFFFu);
    num[root] = 0;
    parent.assign(1, 0u);
    for (size_t q = 0; q < order.size(); q++)
        for (uint32_t c : kids[order[q]]) { num[c] = (uint32_t)order.size(); order.push_back(c); parent.push_back(num[order[q]]); }
    for (size_t i = 0; i < id.size(); i++)
        if (num[i] == 0xFFFFFFFFu) throw bad(line_of[i], "a cycle: taxon " + to_string(id[i]) + " never reaches the root");
    ids.clear(); number.clear();
    for (uint32_t i : order) { number[id[i]] = (uint32_t)ids.size(); ids.push_back(id[i]); }
}
// --color-taxa FILE: one taxon id per reference of --color-refs, in its order; empty lines are skipped and do not count, as in that list
static vector<uint32_t> color_taxa_parse_file(const string& path, const unordered_map<int64_t, uint32_t>& number, size_t n_refs) {
    ifstream in(path);
    if (!in) throw runtime_error("--color-taxa: cannot read " + path);
    vector<uint32_t> out;
    string line;
    for (size_t n = 1; getline(in, line); n++) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        int64_t a = 0;
        if (!taxon_id(line, a)) throw runtime_error("--color-taxa: " + path + " line " + to_string(n) + ": wants one taxon id, an integer");
        auto it = number.find(a);
        if (it == number.end()) throw runtime_error("--color-taxa: " + path + " line " + to_string(n) + ": taxon " + to_string(a) + " is not in the file of --taxonomy");
        if (out.size() == n_refs) throw runtime_error("--color-taxa: " + path + " line " + to_string(n) + ": a taxon more than the " + to_string(n_refs) + " references --color-refs names");
        out.push_back(it->second);
    }
    if (out.size() != n_refs) throw runtime_error("--color-taxa: " + path + " has " + to_string(out.size()) + " taxa, --color-refs names " + to_string(n_refs) + " references");
    return out;
}
// the labelling of --label-unitigs FASTA --labels FILE, in the index's unitig numbers (fin_index_unitig_numbers); *n_labels = the largest label + 1
static vector<uint32_t> load_labelling(const FinimizerIndex& index, const string& fasta, const string& file, uint32_t* n_labels) {
    string bases; vector<uint64_t> offsets{0};
    {
        SeqReader reader(fasta);
        while (reader.get_next_read_to_buffer() > 0) { bases += reader.read_buf; offsets.push_back(bases.size()); }
    }
    const size_t n = offsets.size() - 1;
    ifstream in(file);
    if (!in) throw runtime_error("Could not open the labels file " + file);
    vector<uint32_t> given;
    string line;
    uint64_t top = 0;
    while (getline(in, line)) {
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        const string where = file + " line " + to_string(given.size() + 1);
        if (given.size() == n) throw runtime_error(where + ": more lines than " + fasta + " has records (" + to_string(n) + ")");
        if (line == "-") { given.push_back(FIN_NO_LABEL); continue; }
        size_t used = 0; unsigned long long v = 0;
        try { v = stoull(line, &used); } catch (...) { used = 0; }
        if (line.empty() || used != line.size() || !isdigit((unsigned char)line[0]) || v >= 0x80000000ull)
            throw runtime_error(where + ": `" + line + "` is neither a label (a number from 0 to 2147483647) nor `-`");
        given.push_back((uint32_t)v);
        if (v + 1 > top) top = v + 1;
    }
    if (given.size() != n) throw runtime_error(file + " ends after line " + to_string(given.size()) + ": " + fasta + " has " + to_string(n) + " records, each needs a line");
    const size_t nu = (size_t)index.number_of_unitigs();
    vector<uint32_t> number(n + 1), labels(nu + 1, FIN_NO_LABEL);
    vector<char> seen(nu + 1, 0);
    char err[512] = {0};
    if (fin_index_unitig_numbers(index.handle(), bases.data(), offsets.data(), n, number.data(), err, sizeof err) != FIN_OK) throw runtime_error(fasta + ": " + err);
    for (size_t i = 0; i < n; i++) {
        if (seen[number[i]]) throw runtime_error(fasta + ": record " + to_string(i) + " is a unitig an earlier record already named");
        seen[number[i]] = 1; labels[number[i]] = given[i];
    }
    *n_labels = (uint32_t)(top ? top : 1);
    return labels;
}
// --pseudoalign FILE: every chunk's reads are pseudoaligned against the colours of --color-refs on the first device (fin_search_batch_pseudoalign) and written as
// lines, by the search stage, in chunk order
static fin_colors* g_colors = nullptr;
static FILE* g_psa_file = nullptr;
static uint64_t g_psa_read0 = 0;
static uint32_t g_psa_permille = 1000;
static vector<uint64_t> g_psa_rows; static vector<fin_read_pseudo> g_psa_heads; static string g_psa_text;
// --paired 1: the query's records are interleaved mates; --pseudoalign, --eqclasses, --color-report and --abundance take fragments (fin_search_batch_*_paired)
static bool g_paired = false; static uint32_t g_pair_mode = FIN_PAIR_ANY; static vector<fin_pair_pseudo> g_pair_heads; static string g_query_name;
static void append_colors(string& t, const uint64_t* row, uint32_t W) {
    bool any = false;
    for (uint32_t w = 0; w < W; w++)
        for (uint64_t x = row[w]; x; x &= x - 1) { if (any) t += ','; t += to_string(64 * w + (uint32_t)__builtin_ctzll(x)); any = true; }
    if (!any) t += '-';
}
static void pseudoalign_chunk(const FinimizerIndex& index, const char* bases, const uint64_t* offsets, uint64_t n_reads, const uint64_t* pair_off) {
    char err[512] = {0};
    const uint32_t W = fin_colors_words(g_colors);
    if (g_paired) {   // (the parser cuts chunks after an even number of records)
        const uint64_t nf = n_reads / 2;
        g_psa_rows.resize((size_t)nf * W + 1); g_pair_heads.resize(nf + 1);
        if (fin_search_batch_pseudoalign_paired(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_colors, g_psa_permille, g_pair_mode, g_psa_rows.data(),
                                                g_pair_heads.data(), nullptr, err, sizeof err) != FIN_OK)
            throw runtime_error(err);
        string& t = g_psa_text;
        t.clear();
        for (uint64_t f = 0; f < nf; f++) {
            const fin_pair_pseudo& S = g_pair_heads[f];
            t += to_string(g_psa_read0 + f); t += '\t'; t += to_string(pair_off[2 * f + 2] - pair_off[2 * f]); t += '\t'; t += to_string(S.n_found); t += '\t';
            t += to_string(S.n_colored); t += '\t'; t += to_string(S.n_colored_first); t += '\t';
            append_colors(t, g_psa_rows.data() + (size_t)f * W, W);
            t += '\n';
        }
        if (!t.empty() && fwrite(t.data(), 1, t.size(), g_psa_file) != t.size()) throw runtime_error("Error writing the pseudoalignment file");
        g_psa_read0 += nf;
        return;
    }
    g_psa_rows.resize((size_t)n_reads * W + 1); g_psa_heads.resize(n_reads + 1);
    if (fin_search_batch_pseudoalign(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_colors, g_psa_permille, g_psa_rows.data(), g_psa_heads.data(), nullptr, err,
                                     sizeof err) != FIN_OK)
        throw runtime_error(err);
    string& t = g_psa_text;
    t.clear();
    for (uint64_t r = 0; r < n_reads; r++) {
        const fin_read_pseudo& S = g_psa_heads[r];
        t += to_string(g_psa_read0 + r); t += '\t'; t += to_string(pair_off[r + 1] - pair_off[r]); t += '\t'; t += to_string(S.n_found); t += '\t';
        t += to_string(S.n_colored); t += '\t';
        append_colors(t, g_psa_rows.data() + (size_t)r * W, W);
        t += '\n';
    }
    if (!t.empty() && fwrite(t.data(), 1, t.size(), g_psa_file) != t.size()) throw runtime_error("Error writing the pseudoalignment file");
    g_psa_read0 += n_reads;
}
// colour `color` for every unitig in which a k-mer of the file's sequences is found.  A sequence of more than COLOR_WINDOW k-mers is cut into windows that overlap
// by k - 1 bases: every k-mer lies in exactly one window, and a window is a read of ordinary length for the search pipeline (a chromosome as one read would be
// one sub-batch, scanned by one wave)
static void color_by_search(const FinimizerIndex& index, const string& fasta, uint32_t color) {
    const uint64_t COLOR_WINDOW = 4096, FLUSH_BASES = 64u << 20;
    const uint64_t k = (uint64_t)index.get_k();
    string bases; vector<uint64_t> offsets{0};
    auto flush = [&]() {
        char err[512] = {0};
        if (offsets.size() > 1 && fin_search_batch_add_colors(index.handle(), bases.data(), offsets.data(), offsets.size() - 1, FIN_MERGED, g_colors, color, err, sizeof err) != FIN_OK)
            throw runtime_error(fasta + ": " + err);
        bases.clear(); offsets.assign(1, 0);
    };
    SeqReader reader(fasta);
    int64_t len;
    while ((len = reader.get_next_read_to_buffer()) > 0) {
        const char* seq = reader.read_buf.data();
        const uint64_t n = (uint64_t)len;
        if (n < k) continue;   // no k-mer
        for (uint64_t at = 0; at + k <= n; at += COLOR_WINDOW) {   // k-mers [at, at + COLOR_WINDOW)
            const uint64_t end = min<uint64_t>(n, at + COLOR_WINDOW + k - 1);
            bases.append(seq + at, (size_t)(end - at)); offsets.push_back(bases.size());
        }
        if (bases.size() >= FLUSH_BASES) flush();
    }
    flush();
}
// --eqclasses FILE / --color-report FILE: one accumulator of equivalence classes for the whole run; every chunk's reads are pseudoaligned and added on the
// first device (fin_search_batch_add_eqclasses), nothing per read comes back; both files are written after the last chunk
static fin_eqclasses* g_eqc = nullptr;
// --eqclasses-in: one classes file, as --eqclasses writes it -- `reads<TAB>n_colours<TAB>c1,c2,...` per class, then at most one line `unaligned<TAB>N` --, parsed
// before the index is loaded (every error names the file and the line) and added to the accumulator once it exists (fin_eqclasses_add_classes_host)
static bool parse_u64(const string& t, uint64_t& out) {
    if (t.empty() || t.size() > 20) return false;
    out = 0;
    for (char ch : t) {
        if (ch < '0' || ch > '9') return false;
        const uint64_t d = (uint64_t)(ch - '0');
        if (out > (UINT64_MAX - d) / 10) return false;
        out = out * 10 + d;
    }
    return true;
}
struct EqClassesFile { string path; vector<uint64_t> rows, reads; uint64_t unaligned = 0; };
static EqClassesFile eqclasses_parse_file(const string& path, uint32_t n_colors) {
    ifstream in(path);
    if (!in.good()) throw runtime_error("--eqclasses-in: error opening file " + path);
    EqClassesFile out;
    out.path = path;
    vector<uint64_t>& rows = out.rows; vector<uint64_t>& reads = out.reads;
    uint64_t& unaligned = out.unaligned;
    const uint32_t W = (n_colors + 63u) / 64u;
    uint64_t line_no = 0;
    bool closed = false;   // the unaligned line was met: nothing may follow
    string line;
    const auto bad = [&](const string& what) { return runtime_error("--eqclasses-in: " + path + " line " + to_string(line_no) + ": " + what); };
    while (getline(in, line)) {
        line_no++;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        if (closed) throw bad("a line behind the `unaligned` line");
        const size_t t1 = line.find('\t');
        if (t1 == string::npos) throw bad("malformed line, `reads<TAB>n_colours<TAB>c1,c2,...` or `unaligned<TAB>N` wanted");
        if (line.compare(0, t1, "unaligned") == 0) {
            if (!parse_u64(line.substr(t1 + 1), unaligned)) throw bad("malformed line, `unaligned<TAB>N` wanted");
            closed = true;
            continue;
        }
        const size_t t2 = line.find('\t', t1 + 1);
        uint64_t n_reads = 0, n_listed = 0;
        if (t2 == string::npos || !parse_u64(line.substr(0, t1), n_reads) || !parse_u64(line.substr(t1 + 1, t2 - t1 - 1), n_listed) || t2 + 1 == line.size())
            throw bad("malformed line, `reads<TAB>n_colours<TAB>c1,c2,...` wanted");
        const size_t at = rows.size();
        rows.resize(at + W, 0);
        uint64_t n_set = 0;
        for (size_t p = t2 + 1; p <= line.size();) {
            size_t q = line.find(',', p);
            if (q == string::npos) q = line.size();
            uint64_t c = 0;
            if (!parse_u64(line.substr(p, q - p), c)) throw bad("malformed line, a colour list `c1,c2,...` wanted");
            if (c >= n_colors) throw bad("colour " + to_string(c) + " is not below the " + to_string(n_colors) + " references of --color-refs");
            if (rows[at + (size_t)(c >> 6)] >> (c & 63) & 1) throw bad("malformed line, colour " + to_string(c) + " is listed twice");
            rows[at + (size_t)(c >> 6)] |= 1ull << (c & 63);
            n_set++;
            p = q + 1;
        }
        if (n_set != n_listed) throw bad("n_colours is " + to_string(n_listed) + ", the list has " + to_string(n_set) + " colours");
        reads.push_back(n_reads);
    }
    return out;
}
// --fragments / --fragment-lengths / --ab-fragment-lengths (with --paired 1): the geometry of every fragment, made on the first device; --fragments' lines are written
// by the search stage in chunk order, the histogram and the effective lengths after the last chunk (include/finito_amd.h: FRAGMENT GEOMETRY)
static fin_fragments* g_frag = nullptr;
static FILE* g_frag_file = nullptr;
static uint64_t g_frag0 = 0;
static vector<fin_fragment> g_frag_buf; static string g_frag_text;
static void fragments_chunk(const FinimizerIndex& index, const char* bases, const uint64_t* offsets, uint64_t n_reads) {
    char err[512] = {0};
    if (g_frag && fin_search_batch_add_fragments(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_frag, err, sizeof err) != FIN_OK) throw runtime_error(err);
    if (!g_frag_file) return;
    const uint64_t nf = n_reads / 2;   // (the parser cuts chunks after an even number of records)
    g_frag_buf.resize(nf + 1);
    if (fin_search_batch_fragments(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_frag_buf.data(), err, sizeof err) != FIN_OK) throw runtime_error(err);
    string& t = g_frag_text;
    t.clear();
    for (uint64_t f = 0; f < nf; f++) {
        const fin_fragment& S = g_frag_buf[f];
        t += to_string(g_frag0 + f); t += '\t'; t += to_string(S.cls & 0xFFu); t += '\t';
        if (S.u == 0xFFFFFFFFu) t += "-\t-\t-";
        else { t += to_string(S.u); t += '\t'; t += to_string(S.start); t += '\t'; t += to_string(S.length); }
        t += '\t'; t += (S.cls >> 10) & 1u ? ((S.cls >> 8) & 1u ? 'R' : 'F') : '-';
        t += '\t'; t += (S.cls >> 11) & 1u ? ((S.cls >> 9) & 1u ? 'R' : 'F') : '-';
        t += '\n';
    }
    if (!t.empty() && fwrite(t.data(), 1, t.size(), g_frag_file) != t.size()) throw runtime_error("Error writing the fragments file");
    g_frag0 += nf;
}
static void eqclasses_add_file(const EqClassesFile& f) {
    char err[512] = {0};
    if (fin_eqclasses_add_classes_host(g_eqc, f.rows.data(), f.reads.data(), f.reads.size(), f.unaligned, err, sizeof err) != FIN_OK)
        throw runtime_error("--eqclasses-in: " + f.path + ": " + err);
}
static void eqclasses_chunk(const FinimizerIndex& index, const char* bases, const uint64_t* offsets, uint64_t n_reads) {
    char err[512] = {0};
    if (g_paired) {
        if (fin_search_batch_add_eqclasses_paired(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_eqc, g_psa_permille, g_pair_mode, err, sizeof err) != FIN_OK) throw runtime_error(err);
        return;
    }
    if (fin_search_batch_add_eqclasses(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_eqc, g_psa_permille, err, sizeof err) != FIN_OK) throw runtime_error(err);
}
// --assign-weights FILE: one assignment accumulator for the whole run; every chunk's reads (or fragments) are pseudoaligned, assigned and counted on the first
// device (fin_search_batch_assign); --assign's lines are written by the search stage in chunk order, --assign-report after the last chunk
static fin_assign* g_asg = nullptr;
static FILE* g_asg_file = nullptr;
static uint64_t g_asg_read0 = 0;
static vector<uint64_t> g_asg_rows; static vector<fin_read_assign> g_asg_heads; static string g_asg_text;
static void assign_chunk(const FinimizerIndex& index, const char* bases, const uint64_t* offsets, uint64_t n_reads) {
    char err[512] = {0};
    const uint32_t W = fin_colors_words(g_colors), unit = g_paired ? (g_pair_mode == FIN_PAIR_BOTH ? 2u : 1u) : 0u;
    const uint64_t n = g_paired ? n_reads / 2 : n_reads;   // (the parser cuts chunks after an even number of records)
    if (g_asg_file) g_asg_rows.resize((size_t)n * W + 1);
    g_asg_heads.resize(n + 1);
    if (fin_search_batch_assign(index.handle(), bases, offsets, n_reads, FIN_MERGED, g_asg, g_psa_permille, unit, g_asg_file ? g_asg_rows.data() : nullptr, g_asg_heads.data(),
                                err, sizeof err) != FIN_OK)
        throw runtime_error(err);
    if (!g_asg_file) return;
    string& t = g_asg_text;
    t.clear();
    for (uint64_t r = 0; r < n; r++) {
        t += to_string(g_asg_read0 + r); t += '\t';
        if (g_asg_heads[r].best == FIN_NO_COLOR) t += '-'; else t += to_string(g_asg_heads[r].best);
        t += '\t';
        append_colors(t, g_asg_rows.data() + (size_t)r * W, W);
        t += '\n';
    }
    if (!t.empty() && fwrite(t.data(), 1, t.size(), g_asg_file) != t.size()) throw runtime_error("Error writing the assignment file");
    g_asg_read0 += n;
}
// the `reads` and `share` columns of a file --abundance wrote: a line per colour, `colour<TAB>reads<TAB>share[<TAB>...]`, colours ascending from 0
static void assign_parse_weights(const string& path, size_t n_refs, vector<double>& reads, vector<double>& share) {
    ifstream in(path);
    if (!in.good()) throw runtime_error("--assign-weights: error opening file " + path);
    string line;
    size_t line_no = 0;
    while (getline(in, line)) {
        line_no++;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const string head = line.substr(0, line.find('\t'));
        if (head == "unaligned" || head == "iterations" || head == "loglik" || head == "bootstraps") continue;
        const auto bad = [&](const string& what) { return runtime_error("--assign-weights: " + path + " line " + to_string(line_no) + ": " + what); };
        vector<string> f;
        for (size_t at = 0;;) { const size_t e = line.find('\t', at); f.push_back(line.substr(at, e == string::npos ? e : e - at)); if (e == string::npos) break; at = e + 1; }
        if (f.size() < 3) throw bad("wants `colour<TAB>reads<TAB>share`");
        if (f[0] != to_string(reads.size())) throw bad("colour " + to_string(reads.size()) + " expected, got `" + f[0] + "`");
        double v[2];
        for (int q = 0; q < 2; q++) {
            size_t used = 0;
            try { v[q] = stod(f[1 + q], &used); } catch (...) { used = 0; }
            if (f[1 + q].empty() || used != f[1 + q].size() || !(v[q] >= 0.0) || !std::isfinite(v[q])) throw bad(string(q ? "share" : "reads") + " is not a finite number >= 0");
        }
        if (v[1] > 1.0) throw bad("share is above 1");
        reads.push_back(v[0]); share.push_back(v[1]);
    }
    if (reads.size() != n_refs)
        throw runtime_error("--assign-weights: " + path + " has " + to_string(reads.size()) + " colours, --color-refs names " + to_string(n_refs) + " references");
}
static bool g_no_text = false;
static uint64_t g_hits_total = 0;   // the accumulator's sum after the previous query file

static int64_t run_fmin_queries_streaming(SeqReader* reader, BlockReader* breader, OutSink& out, const FinimizerIndex& index, const string& stats_filename) {
    const int64_t k = index.get_k();
    const bool gpu_text = getenv("FINITO_HOST_FORMAT") == nullptr;   // (FINITO_HOST_FORMAT=1: format the text on the host as round 1 did)
    // chunks of 48 MB of bases (about 4*10^7 k-mers, half a GB of text), four in flight: page-locking host memory costs about
    // 0.15 s per GB, so the stages' buffers are kept small and reused
    const size_t BATCH_BASES = 48u << 20;
    constexpr int N_CHUNKS = 4;
    Chunk chunks[N_CHUNKS];
    BlockingQueue<Chunk*> free_q, search_q, format_q;
    for (auto& c : chunks) free_q.push(&c);
    exception_ptr first_error; mutex err_mu;
    auto note_error = [&]() { lock_guard<mutex> g(err_mu); if (!first_error) first_error = current_exception(); };
    atomic<bool> stop{false};
    atomic<int64_t> t_parse{0}, t_search{0}, t_write{0};   // busy time of the three stages (FINITO_TIMING=1 prints them)

    // stage 1: parse reads into page-locked chunks
    thread parser([&]() {
        bool more = true;
        try {
            while (breader && more && !stop.load()) {   // uncompressed input: whole blocks, parsed by all threads
                Chunk* c = free_q.pop();
                c->failed = false; c->n_bases = 0; c->positive = 0; c->positive_fwd = 0; c->positive_rev = 0;
                if (!c->bases.p) {   // a page-locked buffer made ready beside the index load, if one is there by now
                    lock_guard<mutex> g(g_prewarmed.mu);
                    if (!g_prewarmed.bases.empty()) { c->bases.p = g_prewarmed.bases.back().first; c->bases.cap = g_prewarmed.bases.back().second; g_prewarmed.bases.pop_back(); }
                }
                const int64_t tp0 = cur_time_micros();
                more = breader->next(BATCH_BASES, [&](size_t nbytes) { return c->bases.get(nbytes); }, c->n_bases, c->offsets);
                t_parse += cur_time_micros() - tp0;
                if (more) search_q.push(c); else free_q.push(c);
            }
            while (!breader && more && !stop.load()) {
                Chunk* c = free_q.pop();
                c->failed = false; c->n_bases = 0; c->offsets.assign(1, 0); c->positive = 0; c->positive_fwd = 0; c->positive_rev = 0;
                char* dst = c->bases.get(BATCH_BASES);
                for (;;) {
                    const int64_t len = reader->get_next_read_to_buffer();
                    if (len == 0) {
                        if (g_paired && (c->offsets.size() - 1) % 2 != 0)   // (every earlier chunk is even: this chunk's parity is the file's)
                            throw runtime_error("--paired 1: " + g_query_name + " has an odd number of records, its last record has no mate");
                        more = false; break;
                    }
                    if (c->n_bases + (size_t)len > c->bases.cap) {   // a read longer than the room that is left: enlarge, keeping the content
                        PinnedBuf bigger; char* nd = bigger.get(c->n_bases + (size_t)len + BATCH_BASES / 4);
                        memcpy(nd, dst, c->n_bases);
                        swap(bigger.p, c->bases.p); swap(bigger.cap, c->bases.cap);
                        dst = nd;
                    }
                    memcpy(dst + c->n_bases, reader->read_buf.data(), (size_t)len);
                    c->n_bases += (size_t)len; c->offsets.push_back(c->n_bases);
                    if (c->n_bases >= BATCH_BASES && (!g_paired || (c->offsets.size() - 1) % 2 == 0)) break;   // (--paired 1: never between two mates)
                }
                if (c->offsets.size() > 1) search_q.push(c); else free_q.push(c);
            }
        } catch (...) { note_error(); stop = true; }
        search_q.push(nullptr);
    });

    // stage 2: the GPU search; results land in the chunk's page-locked pair buffer
    int64_t search_wait_micros = 0, t_first = -1;
    thread searcher([&]() {
        for (;;) {
            const int64_t tw = cur_time_micros();
            Chunk* c = search_q.pop();
            if (t_first >= 0) search_wait_micros += cur_time_micros() - tw;
            if (!c) break;
            if (t_first < 0) t_first = cur_time_micros();
            const int64_t ts0 = cur_time_micros();
            try {
                if (!stop.load()) {
                    const uint64_t n_reads = c->offsets.size() - 1;
                    c->pair_off.resize(n_reads + 1); c->pair_off[0] = 0;
                    for (uint64_t r = 0; r < n_reads; r++) {
                        const int64_t len = (int64_t)(c->offsets[r + 1] - c->offsets[r]);
                        c->pair_off[r + 1] = c->pair_off[r] + (uint64_t)(len >= k ? len - k + 1 : 0);
                    }
                    if (g_no_text) {   // the profile / the coverage / the segments are all this chunk is searched for
                        if (g_hits) index.add_unitig_hits(c->bases.get(0), c->offsets.data(), n_reads, g_hits);
                        if (g_cover) add_cover_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                        if (g_depth) add_depth_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                        if (g_links) add_links_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                        if (g_pileup) add_pileup_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                        if (g_seg_file) c->positive = segments_chunk(index, c->bases.get(0), c->offsets.data(), n_reads, c->pair_off[n_reads]);
                        if (g_rs_file) c->positive = read_summary_chunk(index, c->bases.get(0), c->offsets.data(), n_reads, c->pair_off.data());
                        if (g_scr_file) screen_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                        if (g_labels) classify_chunk(index, c->bases.get(0), c->offsets.data(), n_reads, c->pair_off.data());
                        if (g_tax) taxa_chunk(index, c->bases.get(0), c->offsets.data(), n_reads, c->pair_off.data());
                        if (g_psa_file) pseudoalign_chunk(index, c->bases.get(0), c->offsets.data(), n_reads, c->pair_off.data());
                        if (g_eqc) eqclasses_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                        if (g_asg) assign_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                        if (g_frag || g_frag_file) fragments_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                    }
                    else {
                        // the text comes from the GPU when it can (one device, every read has a k-mer), else the pairs do
                        if (!c->text) {
                            lock_guard<mutex> g(g_prewarmed.mu);
                            if (!g_prewarmed.texts.empty()) { c->text = g_prewarmed.texts.back(); g_prewarmed.texts.pop_back(); }
                        }
                        if (!c->text) c->text = fin_text_create();
                        c->as_text = gpu_text && c->text && index.search_batch_text(c->bases.get(0), c->offsets.data(), n_reads, c->text, c->positive);
                        if (!c->as_text) {
                            int32_t* pairs = (int32_t*)c->pairs.get((size_t)(2 * c->pair_off[n_reads] + 2) * sizeof(int32_t));
                            index.search_batch_into(c->bases.get(0), c->offsets.data(), n_reads, pairs, c->positive);
                        }
                        if (g_hits) index.add_unitig_hits(c->bases.get(0), c->offsets.data(), n_reads, g_hits);   // (a second pass over the chunk on the device: the text is what bounds this loop)
                        if (g_cover) add_cover_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                        if (g_depth) add_depth_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                        if (g_links) add_links_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                        if (g_pileup) add_pileup_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                        if (g_seg_file) (void)segments_chunk(index, c->bases.get(0), c->offsets.data(), n_reads, c->pair_off[n_reads]);
                        if (g_rs_file) (void)read_summary_chunk(index, c->bases.get(0), c->offsets.data(), n_reads, c->pair_off.data());
                        if (g_scr_file) screen_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                        if (g_labels) classify_chunk(index, c->bases.get(0), c->offsets.data(), n_reads, c->pair_off.data());
                        if (g_tax) taxa_chunk(index, c->bases.get(0), c->offsets.data(), n_reads, c->pair_off.data());
                        if (g_psa_file) pseudoalign_chunk(index, c->bases.get(0), c->offsets.data(), n_reads, c->pair_off.data());
                        if (g_eqc) eqclasses_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                        if (g_asg) assign_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                        if (g_frag || g_frag_file) fragments_chunk(index, c->bases.get(0), c->offsets.data(), n_reads);
                    }
                    if (g_strand_counts) {
                        c->positive_fwd = index.count_found_one_strand(c->bases.get(0), c->offsets.data(), n_reads);
                        // rc(read) for every read (sbwt::get_rc, search_fmin.hh:50), same offsets
                        c->rc.resize(c->n_bases + 1);
                        const char* src = c->bases.get(0);
#pragma omp parallel for schedule(static)
                        for (int64_t r = 0; r < (int64_t)n_reads; r++) {
                            const uint64_t a = c->offsets[(size_t)r], b = c->offsets[(size_t)r + 1];
                            for (uint64_t i = a; i < b; i++) {
                                const char ch = src[b - 1 - (i - a)];
                                char o2 = ch;
                                switch (ch) { case 'A': o2 = 'T'; break; case 'C': o2 = 'G'; break; case 'G': o2 = 'C'; break; case 'T': o2 = 'A'; break;
                                              case 'a': o2 = 't'; break; case 'c': o2 = 'g'; break; case 'g': o2 = 'c'; break; case 't': o2 = 'a'; break; default: break; }
                                c->rc[(size_t)i] = o2;
                            }
                        }
                        c->positive_rev = index.count_found_one_strand(c->rc.data(), c->offsets.data(), n_reads);
                    }
                } else c->failed = true;
            } catch (...) { note_error(); stop = true; c->failed = true; }
            t_search += cur_time_micros() - ts0;
            format_q.push(c);
        }
        format_q.push(nullptr);
    });

    // stage 3 (this thread + OpenMP team): text "(u,p) (u,p)...\n" per read, search_fmin.hh:62-65, written in input order
    int64_t number_of_queries = 0; uint64_t total_positive = 0, kmers_count = 0, kmers_count_rev = 0;
    Team team(fin_host_threads());
    const int nt = team.n;
    vector<unique_ptr<char[]>> part(nt); vector<size_t> part_cap(nt, 0), part_len(nt, 0);
    int64_t t_last = -1;
    for (;;) {
        Chunk* c = format_q.pop();
        if (!c) break;
        const int64_t tw0 = cur_time_micros();
        if (!c->failed && !stop.load()) {
            try {
                const uint64_t n_reads = c->offsets.size() - 1;
                const vector<uint64_t>& pair_off = c->pair_off;
                number_of_queries += (int64_t)pair_off[n_reads];
                total_positive += c->positive; kmers_count += c->positive_fwd; kmers_count_rev += c->positive_rev;
                if (g_no_text) { t_last = cur_time_micros(); t_write += t_last - tw0; free_q.push(c); continue; }
                if (c->as_text) {   // already text: all threads write their slice of it
                    const char* tp = fin_text_data(c->text); const uint64_t tn = fin_text_size(c->text);
                    // (pwrite by all threads; appending through a shared mapping was tried and is slower: 1.1 s against 0.9 s for 5.2 GB
                    //  on tmpfs, 2.3 s against 0.7 s on a disk-backed file)
                    if (out.seekable) {
                        team.run([&](int t, int tt) { const auto sh = Team::share((size_t)tn, t, tt); OutSink::write_all(out.fd, tp + sh.first, sh.second - sh.first, (int64_t)(out.pos + sh.first)); });
                        out.pos += tn;
                    } else OutSink::write_all(out.fd, tp, (size_t)tn, -1);
                    t_last = cur_time_micros();
                    t_write += t_last - tw0;
                    free_q.push(c);
                    continue;
                }
                const int32_t* pairs = (const int32_t*)c->pairs.get(0);
                vector<uint64_t> cut(nt + 1, n_reads);
                cut[0] = 0;
                for (int t = 1; t < nt; t++)
                    cut[t] = (uint64_t)(lower_bound(pair_off.begin(), pair_off.end(), pair_off[n_reads] * (uint64_t)t / (uint64_t)nt) - pair_off.begin());
                for (int t = 1; t <= nt; t++) cut[t] = min<uint64_t>(max(cut[t], cut[t - 1]), n_reads);
                team.run([&](int t, int) {
                    const uint64_t lo = cut[t], hi = cut[t + 1];
                    const size_t need = (size_t)(pair_off[hi] - pair_off[lo]) * 24 + 2 * (size_t)(hi - lo) + 16;
                    if (need > part_cap[t]) { part[t].reset(new char[need + need / 8]); part_cap[t] = need + need / 8; }
                    char* q = part[t].get();
                    for (uint64_t r = lo; r < hi; r++) q += fin_format_pairs(pairs + 2 * pair_off[r], (int64_t)(pair_off[r + 1] - pair_off[r]), q);
                    part_len[t] = (size_t)(q - part[t].get());
                });
                if (out.seekable)
                    team.run([&](int t, int) {
                        uint64_t at = out.pos;
                        for (int i = 0; i < t; i++) at += part_len[i];
                        OutSink::write_all(out.fd, part[t].get(), part_len[t], (int64_t)at);
                    });
                if (out.seekable) { for (int t = 0; t < nt; t++) out.pos += part_len[t]; }
                else for (int t = 0; t < nt; t++) OutSink::write_all(out.fd, part[t].get(), part_len[t], -1);
            } catch (...) { note_error(); stop = true; }
        }
        t_last = cur_time_micros();
        t_write += t_last - tw0;
        free_q.push(c);
    }
    parser.join(); searcher.join();
    if (getenv("FINITO_TIMING"))
        cerr << "[timing] stage busy seconds: parse " << t_parse.load() * 1e-6 << "  search(+PCIe" << (gpu_text ? "+GPU text" : "") << ") " << t_search.load() * 1e-6
             << "  " << (gpu_text ? "write " : "format+write ") << t_write.load() * 1e-6 << endl;
    if (first_error) rethrow_exception(first_error);
    if (g_no_text && g_hits) {   // no pairs came back: the found k-mers of this file are what the accumulator's sum grew by (with --segments alone: their lengths)
        char err[512] = {0};
        uint64_t tot = 0;
        if (fin_hits_download(g_hits, nullptr, &tot, err, sizeof err) != FIN_OK) throw runtime_error(err);
        total_positive = tot - g_hits_total; g_hits_total = tot;
    }
    // the reference's timed region is search + formatting + printing per read; here: first chunk entering the search until the last
    // chunk is written, minus the time the search stage sat waiting for the parser
    int64_t total_micros = t_first >= 0 && t_last >= 0 ? t_last - t_first - search_wait_micros : 0;
    if (total_micros < 0) total_micros = 0;
    write_log("k " + to_string(k));
    write_log("us/query: " + to_string(number_of_queries ? (double)total_micros / (double)number_of_queries : 0.0) + " (excluding I/O etc)");
    if (g_strand_counts) {   // search_fmin.hh:75-76
        write_log("Found kmers: " + to_string(kmers_count));
        write_log("Found kmers reverse : " + to_string(kmers_count_rev));
    }
    write_log("Total found kmers: " + to_string(total_positive));
    ofstream statsfile(stats_filename, ios::app);
    // (the reference's second field is kmers_count + kmers_count_rev, search_fmin.hh:81; without --strand-counts: the merged count)
    statsfile << to_string(k) + "," + to_string(g_strand_counts ? kmers_count + kmers_count_rev : total_positive) + "," + to_string(number_of_queries);
    return number_of_queries;
}

// --color-similarity / --color-similarity-covered: the colour matrix times itself on the first GPU (fin_colors_shared), over the unitigs' k-mers (cov null) or the
// found k-mers of a bitmap -- `a<TAB>b<TAB>size_a<TAB>size_b<TAB>shared` per pair a < b that shares anything, then `identical<TAB>c1,c2,...` per group of equal columns
static void write_color_similarity(const string& path, fin_cover* cov, size_t nc) {
    char err[512] = {0};
    vector<uint64_t> s(nc * nc + 1);
    if (fin_colors_shared(g_colors, cov, nullptr, s.data(), err, sizeof err) != FIN_OK) throw runtime_error(err);
    string text;
    for (size_t a = 0; a < nc; a++)
        for (size_t b = a + 1; b < nc; b++) {
            if (s[a * nc + b] == 0) continue;
            text += to_string(a); text += '\t'; text += to_string(b);
            for (uint64_t v : {s[a * nc + a], s[b * nc + b], s[a * nc + b]}) { text += '\t'; text += to_string(v); }
            text += '\n';
        }
    vector<char> seen(nc, 0);
    for (size_t a = 0; a < nc; a++) {
        const uint64_t d = s[a * nc + a];
        if (seen[a] || d == 0) continue;
        string line = "identical\t" + to_string(a);
        size_t members = 1;
        for (size_t b = a + 1; b < nc; b++)
            if (s[a * nc + b] == d && s[b * nc + b] == d) { seen[b] = 1; members++; line += ','; line += to_string(b); }
        if (members >= 2) { text += line; text += '\n'; }
    }
    ofstream cf(path, ios::binary | ios::trunc);
    cf.write(text.data(), (streamsize)text.size());
    if (!cf) throw runtime_error("Error writing to file: " + path);
}

static int search_fmin(int argc, char** argv) {
    int64_t micros_start = cur_time_micros();
    Opts o = parse(argc, argv, {{"o", "out-file"}, {"i", "index-file"}, {"q", "query-file"}}, {"out-file", "index-file", "query-file", "device", "gpus", "strand-counts", "unitig-counts", "unitig-coverage", "unitig-depth", "min-depth", "pileup", "variants", "pileup-max-mismatch", "min-alt", "min-alt-permille", "segments", "read-summary", "screen", "min-found", "min-permille", "screen-invert", "label-unitigs", "labels", "classify", "label-report", "class-min-found", "class-min-permille", "class-min-margin", "color-refs", "colors-out", "color-coverage", "depth-histogram", "depth-bins", "depth-bin-width", "color-depth-histogram", "color-depth-quantiles", "color-similarity", "color-similarity-covered", "compact-colors", "color-sets-out", "taxonomy", "color-taxa", "taxa", "taxon-report", "taxa-confidence", "taxa-min-found", "pseudoalign", "pseudo-permille", "eqclasses", "color-report", "eq-max-classes", "eqclasses-in", "eqclasses-unaligned", "abundance", "ab-lengths", "ab-max-iters", "ab-tol", "ab-bootstraps", "ab-seed", "assign-weights", "assign-threshold", "assign", "assign-report", "paired", "pair-both", "fragments", "fragment-lengths", "fragment-bins", "fragment-bin-width", "ab-fragment-lengths", "ref-paths", "ref-depth", "ref-window", "ref-variants", "links", "max-links", "links-min-count", "no-text"});
    if (argc == 1 || o.help) { cerr << SEARCH_HELP << endl; exit(1); }
    g_strand_counts = o.has("strand-counts") && o.get("strand-counts") != "0" && o.get("strand-counts") != "false";
    g_no_text = o.has("no-text") && o.get("no-text") != "0" && o.get("no-text") != "false";
    if (o.has("color-similarity-covered") && !o.has("color-similarity")) throw runtime_error("--color-similarity-covered is only legal together with --color-similarity");
    if (g_no_text && !o.has("unitig-counts") && !o.has("unitig-coverage") && !o.has("unitig-depth") && !o.has("pileup") && !o.has("variants") && !o.has("segments") && !o.has("read-summary") && !o.has("screen") && !o.has("classify") && !o.has("label-report") && !o.has("colors-out") && !o.has("pseudoalign") && !o.has("eqclasses") && !o.has("color-report") && !o.has("abundance") && !o.has("assign-weights") && !o.has("color-coverage") && !o.has("color-similarity") && !o.has("taxa") && !o.has("taxon-report") && !o.has("depth-histogram") && !o.has("color-depth-histogram") && !o.has("color-depth-quantiles") && !o.has("fragments") && !o.has("fragment-lengths") && !o.has("ref-depth") && !o.has("ref-variants") && !o.has("links"))
        throw runtime_error("--no-text 1 is only legal together with --unitig-counts, --unitig-coverage, --unitig-depth, --pileup, --variants, --segments, --read-summary, --screen, --classify, --label-report, --colors-out, --pseudoalign, --eqclasses, --color-report, --abundance, --depth-histogram, --color-depth-histogram, --color-depth-quantiles, --fragments, --fragment-lengths or --links (the run would have no result)");
    if ((o.has("pseudoalign") || o.has("colors-out")) && !o.has("color-refs")) throw runtime_error("--pseudoalign and --colors-out want colours: --color-refs LIST");
    if ((o.has("eqclasses") || o.has("color-report") || o.has("abundance")) && !o.has("color-refs")) throw runtime_error("--eqclasses, --color-report and --abundance want colours: --color-refs LIST");
    if (o.has("color-coverage") && !o.has("color-refs")) throw runtime_error("--color-coverage wants colours: --color-refs LIST");
    if ((o.has("color-depth-histogram") || o.has("color-depth-quantiles")) && !o.has("color-refs")) throw runtime_error("--color-depth-histogram and --color-depth-quantiles want colours: --color-refs LIST");
    if ((o.has("color-similarity") || o.has("color-similarity-covered")) && !o.has("color-refs")) throw runtime_error("--color-similarity and --color-similarity-covered want colours: --color-refs LIST");
    const bool compact_colors = o.has("compact-colors") && o.get("compact-colors") != "0" && o.get("compact-colors") != "false";
    if (compact_colors && !o.has("color-refs")) throw runtime_error("--compact-colors 1 wants colours: --color-refs LIST");
    if (o.has("color-sets-out") && !compact_colors) throw runtime_error("--color-sets-out is only legal together with --compact-colors 1");
    for (const char* name : {"color-coverage", "color-similarity", "taxonomy"})
        if (compact_colors && o.has(name))
            throw runtime_error(string("--compact-colors 1 is not available with --") + name + ": coverage, shared k-mers and taxonomy read the dense colour matrix (fin_colors_expand), over sets they are not built");
    for (const char* name : {"color-depth-histogram", "color-depth-quantiles"})
        if (compact_colors && o.has(name))
            throw runtime_error(string("--compact-colors 1 is not available with --") + name + ": the depth histograms read the dense colour matrix (fin_colors_expand), over sets they are not built");
    // the bins of --depth-histogram, --color-depth-histogram and --color-depth-quantiles: bin(d) = min(d / D, B - 1)
    const bool dh_asked = o.has("depth-histogram") || o.has("color-depth-histogram") || o.has("color-depth-quantiles");
    if ((o.has("depth-bins") || o.has("depth-bin-width")) && !dh_asked) throw runtime_error("--depth-bins and --depth-bin-width are only legal together with --depth-histogram, --color-depth-histogram or --color-depth-quantiles");
    auto dh_number = [&](const char* name, unsigned long long dflt, unsigned long long top) -> uint32_t {
        if (!o.has(name)) return (uint32_t)dflt;
        const string v = o.get(name);
        size_t used = 0; unsigned long long t = 0;
        try { t = stoull(v, &used); } catch (...) { used = 0; }
        if (v.empty() || used != v.size() || v[0] == '-' || t < 1 || t > top) throw runtime_error(string("--") + name + " wants a number from 1 to " + to_string(top));
        return (uint32_t)t;
    };
    const uint32_t dh_bins = dh_number("depth-bins", 256, FIN_DEPTH_HIST_MAX_BINS), dh_width = dh_number("depth-bin-width", 1, 0xFFFFFFFFull);
    // --links FILE [--max-links N] [--links-min-count C]: the numbers are refused before the index is loaded
    for (const char* name : {"max-links", "links-min-count"})
        if (o.has(name) && !o.has("links")) throw runtime_error(string("--") + name + " is only legal together with --links");
    auto links_number = [&](const char* name, unsigned long long dflt, unsigned long long top) -> uint64_t {
        if (!o.has(name)) return dflt;
        const string v = o.get(name);
        size_t used = 0; unsigned long long t = 0;
        try { t = stoull(v, &used); } catch (...) { used = 0; }
        if (v.empty() || used != v.size() || v[0] == '-' || t < 1 || t > top) throw runtime_error(string("--") + name + " wants a number from 1 to " + to_string(top));
        return t;
    };
    const uint64_t max_links = links_number("max-links", 1ull << 20, FIN_LINKS_MAX), links_min_count = links_number("links-min-count", 1, ~0ull);
    g_paired = o.has("paired") && o.get("paired") != "0" && o.get("paired") != "false";
    const bool pair_both = o.has("pair-both") && o.get("pair-both") != "0" && o.get("pair-both") != "false";
    if (g_paired && !o.has("color-refs")) throw runtime_error("--paired 1 wants colours: --color-refs LIST (fragments are what --pseudoalign, --eqclasses, --color-report and --abundance then take)");
    if (pair_both && !g_paired) throw runtime_error("--pair-both 1 is only legal together with --paired 1");
    g_pair_mode = pair_both ? FIN_PAIR_BOTH : FIN_PAIR_ANY;
    // --fragments, --fragment-lengths, --ab-fragment-lengths: all three want --paired 1; the bins as --depth-bins; everything is refused before the index is loaded
    const bool ab_frag = o.has("ab-fragment-lengths") && o.get("ab-fragment-lengths") != "0" && o.get("ab-fragment-lengths") != "false";
    const bool frag_asked = o.has("fragments") || o.has("fragment-lengths") || ab_frag;
    for (const char* name : {"fragments", "fragment-lengths"})
        if (o.has(name) && !g_paired) throw runtime_error(string("--") + name + " wants interleaved mates: --paired 1");
    if (ab_frag && !g_paired) throw runtime_error("--ab-fragment-lengths 1 wants interleaved mates: --paired 1");
    if (ab_frag && !(o.has("abundance") && o.has("ab-lengths"))) throw runtime_error("--ab-fragment-lengths 1 wants --abundance FILE and --ab-lengths FILE (the references' lengths in bases)");
    if (ab_frag && o.has("ab-bootstraps")) throw runtime_error("--ab-fragment-lengths 1 is not available with --ab-bootstraps");
    for (const char* name : {"fragment-bins", "fragment-bin-width"})
        if (o.has(name) && !o.has("fragment-lengths") && !ab_frag) throw runtime_error(string("--") + name + " is only legal together with --fragment-lengths or --ab-fragment-lengths 1");
    const uint32_t frag_bins = dh_number("fragment-bins", 1024, FIN_FRAG_MAX_BINS), frag_width = dh_number("fragment-bin-width", 1, 0xFFFFFFFFull);
    if (ab_frag && frag_width != 1) throw runtime_error("--ab-fragment-lengths 1 wants --fragment-bin-width 1: effective lengths are read from a histogram of single lengths");
    const bool eq_asked = o.has("eqclasses") || o.has("color-report") || o.has("abundance");
    const bool asg_asked = o.has("assign-weights");
    const bool tax_asked = o.has("taxa") || o.has("taxon-report");
    if (tax_asked && !(o.has("taxonomy") && o.has("color-taxa") && o.has("color-refs"))) throw runtime_error("--taxa and --taxon-report want a taxonomy over colours: --color-refs LIST --taxonomy FILE --color-taxa FILE");
    for (const char* name : {"taxonomy", "color-taxa", "taxa-confidence", "taxa-min-found"})
        if (o.has(name) && !tax_asked) throw runtime_error(string("--") + name + " is only legal together with --taxa or --taxon-report");
    if (tax_asked && g_paired) throw runtime_error("--taxa and --taxon-report call reads, not fragments: not together with --paired 1");
    if (asg_asked && !o.has("color-refs")) throw runtime_error("--assign-weights wants colours: --color-refs LIST");
    if (asg_asked && !o.has("assign") && !o.has("assign-report")) throw runtime_error("--assign-weights wants a result: --assign FILE and / or --assign-report FILE");
    for (const char* name : {"assign", "assign-report", "assign-threshold"})
        if (o.has(name) && !asg_asked) throw runtime_error(string("--") + name + " is only legal together with --assign-weights");
    if (o.has("color-refs") && !o.has("pseudoalign") && !o.has("colors-out") && !eq_asked && !asg_asked && !o.has("color-coverage") && !o.has("color-similarity") && !tax_asked && !o.has("color-depth-histogram") && !o.has("color-depth-quantiles") && !frag_asked) throw runtime_error("--color-refs is only legal together with --pseudoalign, --colors-out, --eqclasses, --color-report, --abundance, --color-depth-histogram or --color-depth-quantiles");
    if (o.has("pseudo-permille") && !o.has("pseudoalign") && !eq_asked && !asg_asked) throw runtime_error("--pseudo-permille is only legal together with --pseudoalign, --eqclasses, --color-report or --abundance");
    if (o.has("eq-max-classes") && !eq_asked) throw runtime_error("--eq-max-classes is only legal together with --eqclasses, --color-report or --abundance");
    if (o.has("eqclasses-in") && !eq_asked) throw runtime_error("--eqclasses-in is only legal together with --eqclasses, --color-report or --abundance");
    if (o.has("eqclasses-unaligned") && !o.has("eqclasses")) throw runtime_error("--eqclasses-unaligned is only legal together with --eqclasses");
    if (o.has("ab-seed") && !o.has("ab-bootstraps")) throw runtime_error("--ab-seed is only legal together with --ab-bootstraps");
    for (const char* name : {"ab-lengths", "ab-max-iters", "ab-tol", "ab-bootstraps"})
        if (o.has(name) && !o.has("abundance") && !(asg_asked && !strcmp(name, "ab-lengths"))) throw runtime_error(string("--") + name + " is only legal together with --abundance");
    if ((o.has("classify") || o.has("label-report")) && !(o.has("label-unitigs") && o.has("labels"))) throw runtime_error("--classify and --label-report want a labelling: --label-unitigs FASTA --labels FILE");
    if ((o.has("label-unitigs") || o.has("labels")) && !o.has("classify") && !o.has("label-report")) throw runtime_error("--label-unitigs and --labels are only legal together with --classify or --label-report");
    for (const char* name : {"class-min-found", "class-min-permille", "class-min-margin"})
        if (o.has(name) && !o.has("label-report")) throw runtime_error(string("--") + name + " is only legal together with --label-report");
    for (const char* name : {"min-found", "min-permille", "screen-invert"})
        if (o.has(name) && !o.has("screen")) throw runtime_error(string("--") + name + " is only legal together with --screen");
    auto u32_option = [&](const char* name, unsigned long long dflt, unsigned long long top) {
        if (!o.has(name)) return (uint32_t)dflt;
        const string v = o.get(name);
        size_t used = 0; unsigned long long t = 0;
        try { t = stoull(v, &used); } catch (...) { used = 0; }
        if (v.empty() || used != v.size() || v[0] == '-' || t > top) throw runtime_error(string("--") + name + " wants a number from 0 to " + to_string(top));
        return (uint32_t)t;
    };
    g_scr_min_found = u32_option("min-found", 1, 0xFFFFFFFFull);
    g_scr_min_permille = u32_option("min-permille", 0, 1000);
    g_cls_min_found = u32_option("class-min-found", 1, 0xFFFFFFFFull);
    g_cls_min_permille = u32_option("class-min-permille", 0, 1000);
    g_cls_min_margin = u32_option("class-min-margin", 0, 0xFFFFFFFFull);
    g_psa_permille = u32_option("pseudo-permille", 1000, 1000);
    g_tax_confidence = u32_option("taxa-confidence", 0, 1000);
    g_tax_min_found = u32_option("taxa-min-found", 1, 0xFFFFFFFFull);
    const uint32_t eq_max_classes = u32_option("eq-max-classes", 1u << 20, 1u << 26);
    if (eq_max_classes == 0) throw runtime_error("--eq-max-classes wants a number from 1 to " + to_string(1u << 26));
    const uint32_t ab_max_iters = u32_option("ab-max-iters", 1000, 100000);
    if (ab_max_iters == 0) throw runtime_error("--ab-max-iters wants a number from 1 to 100000");
    uint32_t ab_bootstraps = 0;             // 0: none asked for
    if (o.has("ab-bootstraps")) {
        try { ab_bootstraps = u32_option("ab-bootstraps", 0, 4096); } catch (const runtime_error&) { ab_bootstraps = 0; }
        if (ab_bootstraps == 0) throw runtime_error("--ab-bootstraps wants a number from 1 to 4096");
    }
    uint64_t ab_seed = 0;
    if (o.has("ab-seed")) {
        const string v = o.get("ab-seed");
        size_t used = 0;
        try { ab_seed = stoull(v, &used); } catch (...) { used = 0; }
        if (v.empty() || used != v.size() || v[0] == '-') throw runtime_error("--ab-seed wants an unsigned 64-bit number");
    }
    auto positive_number = [](const string& v, bool zero_too, double& out) {   // a finite number above 0 (or from 0 on), nothing behind it
        size_t used = 0;
        try { out = stod(v, &used); } catch (...) { return false; }
        return used == v.size() && std::isfinite(out) && (out > 0.0 || (zero_too && out == 0.0));
    };
    double ab_tol = 1e-6;
    if (o.has("ab-tol") && !positive_number(o.get("ab-tol"), true, ab_tol)) throw runtime_error("--ab-tol wants a number from 0 on");
    vector<string> color_refs;
    if (o.has("color-refs")) {
        color_refs = readlines(o.get("color-refs"));
        if (color_refs.empty()) throw runtime_error("--color-refs: " + o.get("color-refs") + " is empty, it names no reference");
        if (color_refs.size() > FIN_MAX_COLORS) throw runtime_error("--color-refs: " + o.get("color-refs") + " names " + to_string(color_refs.size()) + " references, at most " + to_string(FIN_MAX_COLORS) + " colours are supported");
    }
    vector<uint32_t> tax_parent, tax_color_taxon;
    if (tax_asked) {
        unordered_map<int64_t, uint32_t> number;
        taxonomy_parse_file(o.get("taxonomy"), g_tax_ids, tax_parent, number);
        tax_color_taxon = color_taxa_parse_file(o.get("color-taxa"), number, color_refs.size());
    }
    const string taxa_file = o.get("taxa", ""), taxrep_file = o.get("taxon-report", "");
    if (!taxa_file.empty()) check_writable(taxa_file);
    if (!taxrep_file.empty()) check_writable(taxrep_file);
    const bool eqc_unaligned = o.has("eqclasses-unaligned") && o.get("eqclasses-unaligned") != "0" && o.get("eqclasses-unaligned") != "false";
    vector<EqClassesFile> eqc_in;
    if (o.has("eqclasses-in")) {
        const vector<string> paths = readlines(o.get("eqclasses-in"));
        if (paths.empty()) throw runtime_error("--eqclasses-in: " + o.get("eqclasses-in") + " is empty, it names no classes file");
        for (auto& f : paths) eqc_in.push_back(eqclasses_parse_file(f, (uint32_t)color_refs.size()));
    }
    g_scr_invert = o.has("screen-invert") && o.get("screen-invert") != "0" && o.get("screen-invert") != "false" ? 1 : 0;
    if (o.has("min-depth") && !o.has("unitig-depth") && !o.has("color-coverage") && !o.has("ref-depth")) throw runtime_error("--min-depth is only legal together with --unitig-depth");
    uint32_t min_depth = 1;
    if (o.has("min-depth")) {
        const string v = o.get("min-depth");
        size_t used = 0; unsigned long long t = 0;
        try { t = stoull(v, &used); } catch (...) { used = 0; }
        if (v.empty() || used != v.size() || v[0] == '-' || t > 0xFFFFFFFFull) throw runtime_error("--min-depth wants a number from 0 to 4294967295");
        min_depth = (uint32_t)t;
    }
    // --ref-paths LIST --ref-depth FILE [--ref-window W] --ref-variants FILE: every refusal before the index is loaded, naming its flag
    for (const char* name : {"ref-depth", "ref-variants"})
        if (o.has(name) && !o.has("ref-paths")) throw runtime_error(string("--") + name + " wants --ref-paths LIST: the references whose coordinates it writes");
    if (o.has("ref-paths") && !o.has("ref-depth") && !o.has("ref-variants")) throw runtime_error("--ref-paths is only legal together with --ref-depth or --ref-variants");
    if (o.has("ref-window") && !o.has("ref-depth")) throw runtime_error("--ref-window is only legal together with --ref-depth");
    uint32_t ref_window = 1000;
    if (o.has("ref-window")) {
        const string v = o.get("ref-window");
        size_t used = 0; unsigned long long t = 0;
        try { t = stoull(v, &used); } catch (...) { used = 0; }
        if (v.empty() || used != v.size() || v[0] == '-' || t < 1 || t > 2147483648ull) throw runtime_error("--ref-window wants a number from 1 to 2147483648");
        ref_window = (uint32_t)t;
    }
    vector<string> ref_paths;
    if (o.has("ref-paths")) {
        ref_paths = readlines(o.get("ref-paths"));
        if (ref_paths.empty()) throw runtime_error("--ref-paths: " + o.get("ref-paths") + " is empty, it names no reference");
        if (o.has("index-file") && ifstream(o.get("index-file") + ".finparts").good()) throw runtime_error("--ref-paths is not available with a partitioned index");
    }
    const bool want_pileup = o.has("pileup") || o.has("variants") || o.has("ref-variants");
    if ((o.has("pileup-max-mismatch") || o.has("min-alt") || o.has("min-alt-permille")) && !want_pileup)
        throw runtime_error("--pileup-max-mismatch, --min-alt and --min-alt-permille are only legal together with --pileup or --variants (or --ref-variants)");
    auto pileup_number = [&](const char* name, unsigned long long dflt, unsigned long long top) -> uint32_t {
        if (!o.has(name)) return (uint32_t)dflt;
        const string v = o.get(name);
        size_t used = 0; unsigned long long t = 0;
        try { t = stoull(v, &used); } catch (...) { used = 0; }
        if (v.empty() || used != v.size() || v[0] == '-' || t > top) throw runtime_error(string("--") + name + " wants a number from 0 to " + to_string(top));
        return (uint32_t)t;
    };
    const uint32_t pileup_max_mm = pileup_number("pileup-max-mismatch", 8, 255), min_alt = pileup_number("min-alt", 2, 0xFFFFFFFFull), min_alt_permille = pileup_number("min-alt-permille", 200, 1000);
    if (g_no_text && g_strand_counts) throw runtime_error("--no-text 1 and --strand-counts 1 do not go together");
    if (!o.has("query-file")) throw runtime_error("Option 'query-file' has no value");
    if (!o.has("index-file")) throw runtime_error("Option 'index-file' has no value");
    string queryfile = o.get("query-file");
    vector<string> query_files;
    bool multi_file = queryfile.size() >= 4 && queryfile.substr(queryfile.size() - 4) == ".txt";
    if (multi_file) query_files = readlines(queryfile); else query_files = {queryfile};
    for (auto& f : query_files) check_readable(f);
    optional<vector<string>> output_files;
    if (o.has("out-file")) {
        string outfile = o.get("out-file");
        if (multi_file) output_files = readlines(outfile); else output_files = vector<string>{outfile};
        for (auto& f : output_files.value()) check_writable(f);
    } else write_log("No output file given, writing to stdout");
    if (output_files.has_value() && output_files.value().size() != query_files.size())
        throw runtime_error("Number of input and output files does not match (" + to_string(query_files.size()) + " vs " +
                            to_string(output_files.value().size()) + ")");
    string index_prefix = o.get("index-file");
    const string counts_file = o.get("unitig-counts", "");
    if (!counts_file.empty()) check_writable(counts_file);
    const string cover_file = o.get("unitig-coverage", "");
    if (!cover_file.empty()) check_writable(cover_file);
    const string depth_file = o.get("unitig-depth", "");
    const string links_file = o.get("links", "");
    if (o.has("links")) check_writable(links_file);
    if (!depth_file.empty()) check_writable(depth_file);
    const string colcov_file = o.get("color-coverage", "");
    if (!colcov_file.empty()) check_writable(colcov_file);
    const string dh_file = o.get("depth-histogram", ""), cdh_file = o.get("color-depth-histogram", ""), cdq_file = o.get("color-depth-quantiles", "");
    for (const string* f : {&dh_file, &cdh_file, &cdq_file}) if (!f->empty()) check_writable(*f);
    const string colsim_file = o.get("color-similarity", ""), colsim_cov_file = o.get("color-similarity-covered", "");
    if (!colsim_file.empty()) check_writable(colsim_file);
    if (!colsim_cov_file.empty()) check_writable(colsim_cov_file);
    const string pileup_file = o.get("pileup", ""), variants_file = o.get("variants", "");
    if (!pileup_file.empty()) check_writable(pileup_file);
    if (!variants_file.empty()) check_writable(variants_file);
    const string refdepth_file = o.get("ref-depth", ""), refvar_file = o.get("ref-variants", "");
    if (!refdepth_file.empty()) check_writable(refdepth_file);
    if (!refvar_file.empty()) check_writable(refvar_file);
    for (auto& f : ref_paths) check_readable(f);
    const string seg_file = o.get("segments", "");
    if (!seg_file.empty()) check_writable(seg_file);
    const string rs_file = o.get("read-summary", "");
    if (!rs_file.empty()) check_writable(rs_file);
    const string scr_file = o.get("screen", "");
    if (!scr_file.empty()) check_writable(scr_file);
    const string cls_file = o.get("classify", ""), report_file = o.get("label-report", "");
    if (!cls_file.empty()) check_writable(cls_file);
    if (!report_file.empty()) check_writable(report_file);
    const string colors_file = o.get("colors-out", ""), psa_file = o.get("pseudoalign", "");
    const string eqc_file = o.get("eqclasses", ""), crep_file = o.get("color-report", ""), ab_file = o.get("abundance", "");
    vector<double> ab_lengths;   // --ab-lengths: one positive number per line, line number = colour; a wrong count is an error before any search
    if (o.has("ab-lengths")) {
        const vector<string> lines = readlines(o.get("ab-lengths"));
        if (lines.size() != color_refs.size())
            throw runtime_error("--ab-lengths: " + o.get("ab-lengths") + " has " + to_string(lines.size()) + " lines, --color-refs names " + to_string(color_refs.size()) + " references");
        ab_lengths.resize(lines.size());
        for (size_t c = 0; c < lines.size(); c++) {
            string v = lines[c];
            if (!v.empty() && v.back() == '\r') v.pop_back();
            if (!positive_number(v, false, ab_lengths[c])) throw runtime_error("--ab-lengths: line " + to_string(c + 1) + " (colour " + to_string(c) + ") is not a finite positive number");
            if (ab_frag && !(ab_lengths[c] >= 1.0 && ab_lengths[c] <= 9007199254740992.0 && ab_lengths[c] == std::floor(ab_lengths[c])))
                throw runtime_error("--ab-fragment-lengths 1: --ab-lengths line " + to_string(c + 1) + " (colour " + to_string(c) + ") is not a length in bases, a whole number from 1");
        }
    }
    // --assign-weights: the weights and thresholds, read before the index is loaded; a wrong colour count is an error before any search
    const string asg_file = o.get("assign", ""), asg_report = o.get("assign-report", "");
    vector<double> asg_w, asg_thr;
    if (asg_asked) {
        vector<double> share;
        assign_parse_weights(o.get("assign-weights"), color_refs.size(), asg_w, share);
        if (!ab_lengths.empty()) for (size_t c = 0; c < asg_w.size(); c++) asg_w[c] = asg_w[c] / ab_lengths[c];
        const string tv = o.get("assign-threshold", "0.5");
        if (tv == "abundance") asg_thr = share;
        else {
            double t = 0.0; size_t used = 0;
            try { t = stod(tv, &used); } catch (...) { used = 0; }
            if (tv.empty() || used != tv.size() || !(t >= 0.0 && t <= 1.0)) throw runtime_error("--assign-threshold wants a number from 0 to 1, or `abundance`");
            asg_thr.assign(asg_w.size(), t);
        }
        if (!asg_file.empty()) check_writable(asg_file);
        if (!asg_report.empty()) check_writable(asg_report);
    }
    if (!ab_file.empty()) check_writable(ab_file);
    const string frag_file = o.get("fragments", ""), fraglen_file = o.get("fragment-lengths", "");
    if (!frag_file.empty()) check_writable(frag_file);
    if (!fraglen_file.empty()) check_writable(fraglen_file);
    if (!eqc_file.empty()) check_writable(eqc_file);
    if (!crep_file.empty()) check_writable(crep_file);
    if (!colors_file.empty()) check_writable(colors_file);
    if (!psa_file.empty()) check_writable(psa_file);
    if (!links_file.empty() && fin_pindex_exists(index_prefix.c_str())) throw runtime_error("--links is not available with a partitioned index");
    cerr << "Loading index..." << endl;
    const int first_dev = stoi(o.get("device", "0"));
    // beside the index load: page-lock the pipeline's buffers (four chunks of 48 MB of bases and of up to 16 bytes of text per k-mer)
    // -- as many as the query files can fill (a run on a few reads must not pin 3 GB), none for a multi-GPU run (its text is formatted on
    // the host), and no more once the searches are done
    atomic<bool> prewarm_stop{false};
    int prewarm_chunks = 4;
    {
        uint64_t qbytes = 0;
        for (auto& f : query_files) { struct stat sb; if (stat(f.c_str(), &sb) == 0) qbytes += (uint64_t)sb.st_size; else qbytes += 1ull << 32; }
        const bool gz = !query_files.empty() && query_files[0].size() > 3 && query_files[0].substr(query_files[0].size() - 3) == ".gz";
        const uint64_t est = gz ? qbytes * 4 : qbytes;   // (bases are at most the file's size; a gzip file inflates about fourfold)
        prewarm_chunks = (int)min<uint64_t>(4, (est + (48u << 20) - 1) / (48u << 20));
        const int want_gpus = o.has("gpus") ? stoi(o.get("gpus")) : fin_device_count() - first_dev;
        if (want_gpus > 1) prewarm_chunks = 0;
    }
    thread prewarm([&]() {
        if (getenv("FINITO_HOST_FORMAT")) return;
        for (int i = 0; i < prewarm_chunks && !prewarm_stop.load(); i++) {
            const size_t nb = (48u << 20) + (48u << 20) / 8 + 4096;
            void* p = fin_host_alloc(nb);
            fin_text* t = fin_text_create();
            if (t && fin_text_reserve(t, 16ull * (48u << 20)) != FIN_OK) { fin_text_free(t); t = nullptr; }
            lock_guard<mutex> g(g_prewarmed.mu);
            if (p) g_prewarmed.bases.push_back({p, nb});
            if (t) g_prewarmed.texts.push_back(t);
        }
    });
    struct Joiner { thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{prewarm};   // (an exception below must not leave the thread running)
    FinimizerIndex index(first_dev);
    int ngpus = o.has("gpus") ? stoi(o.get("gpus")) : fin_device_count() - first_dev;
    if (ngpus > 1) index.use_devices(first_dev, ngpus);
    const int64_t t_l0 = cur_time_micros();
    index.load(index_prefix);
    const int64_t t_l1 = cur_time_micros();
    if (!counts_file.empty() && index.partitioned()) throw runtime_error("--unitig-counts is not available with a partitioned index");
    if (!cover_file.empty() && index.partitioned()) throw runtime_error("--unitig-coverage is not available with a partitioned index");
    if (!depth_file.empty() && index.partitioned()) throw runtime_error("--unitig-depth is not available with a partitioned index");
    if (want_pileup && index.partitioned()) throw runtime_error("--pileup and --variants are not available with a partitioned index");
    if (!seg_file.empty() && index.partitioned()) throw runtime_error("--segments is not available with a partitioned index");
    if (!rs_file.empty() && index.partitioned()) throw runtime_error("--read-summary is not available with a partitioned index");
    if (!scr_file.empty() && index.partitioned()) throw runtime_error("--screen is not available with a partitioned index");
    if (!cls_file.empty() && index.partitioned()) throw runtime_error("--classify is not available with a partitioned index");
    if (!report_file.empty() && index.partitioned()) throw runtime_error("--label-report is not available with a partitioned index");
    if (dh_asked && index.partitioned()) throw runtime_error("--depth-histogram, --color-depth-histogram and --color-depth-quantiles are not available with a partitioned index");
    if (!colcov_file.empty() && index.partitioned()) throw runtime_error("--color-coverage is not available with a partitioned index");
    if (!color_refs.empty() && index.partitioned()) throw runtime_error("--color-refs is not available with a partitioned index");
    if (!ref_paths.empty() && index.partitioned()) throw runtime_error("--ref-paths is not available with a partitioned index");
    if (frag_asked && index.partitioned()) throw runtime_error("--fragments, --fragment-lengths and --ab-fragment-lengths are not available with a partitioned index");
    index.to_device();
    struct FragOwner { ~FragOwner() { if (g_frag_file) fclose(g_frag_file); g_frag_file = nullptr; fin_fragments_free(g_frag); g_frag = nullptr; } } frag_owner;
    if (!fraglen_file.empty() || ab_frag) {
        char err[512] = {0};
        if (fin_fragments_create(index.handle(), first_dev, frag_bins, frag_width, &g_frag, err, sizeof err) != FIN_OK) throw runtime_error(err);
    }
    if (!frag_file.empty()) {
        g_frag_file = fopen(frag_file.c_str(), "wb");
        if (!g_frag_file) throw runtime_error("Error writing to file: " + frag_file);
    }
    struct HitsOwner { ~HitsOwner() { fin_hits_free(g_hits); g_hits = nullptr; } } hits_owner;
    if (!counts_file.empty() || (g_no_text && seg_file.empty() && rs_file.empty())) {   // (with --segments the found k-mers are the sum of the segments' lengths, with --read-summary the sum of `found`)
        char err[512] = {0};
        if (fin_hits_create(index.handle(), first_dev, &g_hits, err, sizeof err) != FIN_OK) throw runtime_error(err);
    }
    struct CoverOwner { ~CoverOwner() { fin_cover_free(g_cover); g_cover = nullptr; } } cover_owner;
    if (!cover_file.empty() || !colcov_file.empty() || !colsim_cov_file.empty()) {   // (--color-coverage and --color-similarity-covered share the bitmap and the depth of --unitig-coverage / --unitig-depth)
        char err[512] = {0};
        if (fin_cover_create(index.handle(), first_dev, &g_cover, err, sizeof err) != FIN_OK) throw runtime_error(err);
    }
    struct DepthOwner { ~DepthOwner() { fin_depth_free(g_depth); g_depth = nullptr; } } depth_owner;
    if (!depth_file.empty() || !colcov_file.empty() || dh_asked || !refdepth_file.empty()) {   // (--ref-depth and the depth histograms share the depth of --unitig-depth / --color-coverage)
        char err[512] = {0};
        if (fin_depth_create(index.handle(), first_dev, &g_depth, err, sizeof err) != FIN_OK) throw runtime_error(err);
    }
    struct LinksOwner { ~LinksOwner() { fin_links_free(g_links); g_links = nullptr; } } links_owner;
    if (!links_file.empty()) {
        char err[512] = {0};
        if (index.partitioned()) throw runtime_error("--links is not available with a partitioned index");
        if (fin_links_create(index.handle(), first_dev, max_links, &g_links, err, sizeof err) != FIN_OK) throw runtime_error(string("--links: ") + err);
    }
    struct PileupOwner { ~PileupOwner() { fin_pileup_free(g_pileup); g_pileup = nullptr; } } pileup_owner;
    if (want_pileup) {
        char err[512] = {0};
        if (fin_pileup_create(index.handle(), first_dev, pileup_max_mm, &g_pileup, err, sizeof err) != FIN_OK) throw runtime_error(err);
    }
    // the references' paths, before the first chunk of reads, one reference file after another: every record whole, as one sequence (ref, record)
    struct RefPathsOwner { ~RefPathsOwner() { fin_refpaths_free(g_refpaths); g_refpaths = nullptr; } } refpaths_owner;
    vector<pair<uint32_t, uint32_t>> ref_ids;
    if (!ref_paths.empty()) {
        char err[512] = {0};
        if (fin_refpaths_create(index.handle(), first_dev, &g_refpaths, err, sizeof err) != FIN_OK) throw runtime_error(err);
        const uint64_t FLUSH_BASES = 64u << 20;
        for (size_t r = 0; r < ref_paths.size(); r++) {
            string bases; vector<uint64_t> offsets{0};
            auto flush = [&]() {
                if (offsets.size() > 1 && fin_search_batch_add_refpaths(index.handle(), bases.data(), offsets.data(), offsets.size() - 1, g_refpaths, err, sizeof err) != FIN_OK)
                    throw runtime_error(ref_paths[r] + ": " + err);
                bases.clear(); offsets.assign(1, 0);
            };
            SeqReader reader(ref_paths[r]);
            int64_t len;
            uint32_t record = 0;
            while ((len = reader.get_next_read_to_buffer()) > 0) {
                bases.append(reader.read_buf.data(), (size_t)len); offsets.push_back(bases.size());
                ref_ids.push_back({(uint32_t)r, record++});
                if (bases.size() >= FLUSH_BASES) flush();
            }
            flush();
        }
        if (fin_refpaths_n_seqs(g_refpaths) != ref_ids.size()) throw runtime_error("--ref-paths: the paths and the records read do not agree");
        write_log("Reference paths: " + to_string(ref_ids.size()) + " records of " + to_string(ref_paths.size()) + " files, " + to_string(fin_refpaths_n_segments(g_refpaths)) +
                  " segments over " + to_string(fin_refpaths_n_slots(g_refpaths)) + " k-mers");
    }
    struct SegOwner { ~SegOwner() { if (g_seg_file) fclose(g_seg_file); g_seg_file = nullptr; } } seg_owner;
    if (!seg_file.empty()) {
        g_seg_file = fopen(seg_file.c_str(), "wb");
        if (!g_seg_file) throw runtime_error("Error writing to file: " + seg_file);
        g_seg_read0 = 0;
    }
    struct ReadSumOwner { ~ReadSumOwner() { if (g_rs_file) fclose(g_rs_file); g_rs_file = nullptr; if (g_scr_file) fclose(g_scr_file); g_scr_file = nullptr; } } rs_owner;
    if (!rs_file.empty()) {
        g_rs_file = fopen(rs_file.c_str(), "wb");
        if (!g_rs_file) throw runtime_error("Error writing to file: " + rs_file);
        g_rs_read0 = 0;
    }
    if (!scr_file.empty()) {
        g_scr_file = fopen(scr_file.c_str(), "wb");
        if (!g_scr_file) throw runtime_error("Error writing to file: " + scr_file);
        g_scr_read0 = 0;
    }
    struct ClassOwner { ~ClassOwner() { if (g_cls_file) fclose(g_cls_file); g_cls_file = nullptr; fin_labels_free(g_labels); g_labels = nullptr; } } class_owner;
    uint32_t n_labels = 0;
    if (!cls_file.empty() || !report_file.empty()) {
        const vector<uint32_t> labels = load_labelling(index, o.get("label-unitigs"), o.get("labels"), &n_labels);
        char err[512] = {0};
        if (fin_labels_create(index.handle(), first_dev, labels.data(), n_labels, &g_labels, err, sizeof err) != FIN_OK) throw runtime_error(err);
        g_cls_report = !report_file.empty();
        g_cls_read0 = 0;
        if (!cls_file.empty()) {
            g_cls_file = fopen(cls_file.c_str(), "wb");
            if (!g_cls_file) throw runtime_error("Error writing to file: " + cls_file);
        }
    }
    struct TaxOwner { ~TaxOwner() { if (g_tax_file) fclose(g_tax_file); g_tax_file = nullptr; fin_taxonomy_free(g_tax); g_tax = nullptr; } } tax_owner;   // (it reads the colours at its creation only: the order of the two frees does not matter)
    struct ColorOwner { ~ColorOwner() { if (g_psa_file) fclose(g_psa_file); g_psa_file = nullptr; if (g_asg_file) fclose(g_asg_file); g_asg_file = nullptr; fin_assign_free(g_asg); g_asg = nullptr; fin_eqclasses_free(g_eqc); g_eqc = nullptr; fin_colors_free(g_colors); g_colors = nullptr; } } color_owner;
    if (!color_refs.empty()) {
        for (auto& f : color_refs) check_readable(f);
        char err[512] = {0};
        if (fin_colors_create(index.handle(), first_dev, (uint32_t)color_refs.size(), &g_colors, err, sizeof err) != FIN_OK) throw runtime_error(err);
        for (size_t c = 0; c < color_refs.size(); c++) color_by_search(index, color_refs[c], (uint32_t)c);
        const size_t nu = (size_t)index.number_of_unitigs();
        const uint32_t W = fin_colors_words(g_colors);
        vector<uint64_t> bits(nu * W + 1);
        uint64_t n_set = 0;
        if (fin_colors_download(g_colors, bits.data(), &n_set, err, sizeof err) != FIN_OK) throw runtime_error(err);
        write_log("Coloured " + to_string(nu) + " unitigs by " + to_string(color_refs.size()) + " references: " + to_string(n_set) + " (unitig, colour) pairs");
        if (!colors_file.empty()) {
            string text;
            for (size_t u = 0; u < nu; u++) { text += to_string(u); text += '\t'; append_colors(text, bits.data() + u * W, W); text += '\n'; }
            ofstream cf(colors_file, ios::binary | ios::trunc);
            cf.write(text.data(), (streamsize)text.size());
            if (!cf) throw runtime_error("Error writing to file: " + colors_file);
        }
        if (!colsim_file.empty()) write_color_similarity(colsim_file, nullptr, color_refs.size());   // (what the references share in the graph, before any read)
        if (compact_colors) {   // every distinct row once, before the first chunk of reads: what follows reads the sets
            if (fin_colors_compact(g_colors, 0, nullptr, err, sizeof err) != FIN_OK) throw runtime_error(string("--compact-colors: ") + err);
            const uint64_t n_sets = fin_colors_n_sets(g_colors);
            cerr << "colour sets\t" << n_sets << "\t" << (uint64_t)nu * W * 8 << "\t" << (uint64_t)nu * 4 + (n_sets + 1) * W * 8 << endl;
            if (o.has("color-sets-out")) {   // PREFIX.set_of.u32: uint32[n_unitigs]; PREFIX.sets.u64: uint64[(n_sets + 1) * W], little-endian, what fin_colors_upload_sets takes
                vector<uint32_t> set_of(nu + 1);
                vector<uint64_t> sets((size_t)(n_sets + 1) * W);
                uint64_t got = 0;
                if (fin_colors_download_sets(g_colors, set_of.data(), sets.data(), n_sets + 1, &got, err, sizeof err) != FIN_OK) throw runtime_error(err);
                const string f1 = o.get("color-sets-out") + ".set_of.u32", f2 = o.get("color-sets-out") + ".sets.u64";
                ofstream a(f1, ios::binary | ios::trunc), b(f2, ios::binary | ios::trunc);
                a.write((const char*)set_of.data(), (streamsize)(nu * 4));
                b.write((const char*)sets.data(), (streamsize)(sets.size() * 8));
                if (!a) throw runtime_error("Error writing to file: " + f1);
                if (!b) throw runtime_error("Error writing to file: " + f2);
            }
        }
        if (tax_asked) {   // every unitig's taxon: the LCA of its colours' taxa, made on the device from the matrix as it stands now
            if (fin_taxonomy_create_from_colors(g_colors, tax_parent.data(), tax_parent.size(), tax_color_taxon.data(), &g_tax, err, sizeof err) != FIN_OK) throw runtime_error(err);
            g_tax_report = !taxrep_file.empty();
            g_tax_read0 = 0;
            if (!taxa_file.empty()) {
                g_tax_file = fopen(taxa_file.c_str(), "wb");
                if (!g_tax_file) throw runtime_error("Error writing to file: " + taxa_file);
            }
        }
        if (!psa_file.empty()) {
            g_psa_file = fopen(psa_file.c_str(), "wb");
            if (!g_psa_file) throw runtime_error("Error writing to file: " + psa_file);
            g_psa_read0 = 0;
        }
        if ((!eqc_file.empty() || !crep_file.empty() || !ab_file.empty()) && fin_eqclasses_create(g_colors, eq_max_classes, &g_eqc, err, sizeof err) != FIN_OK) throw runtime_error(err);
        if (g_eqc) for (auto& f : eqc_in) eqclasses_add_file(f);   // the earlier runs' classes, before the first chunk
        if (asg_asked) {
            if (fin_assign_create(g_colors, asg_w.data(), asg_thr.data(), &g_asg, err, sizeof err) != FIN_OK) throw runtime_error(string("--assign-weights: ") + err);
            if (!asg_file.empty()) {
                g_asg_file = fopen(asg_file.c_str(), "wb");
                if (!g_asg_file) throw runtime_error("Error writing to file: " + asg_file);
                g_asg_read0 = 0;
            }
        }
    }
    if (getenv("FINITO_TIMING"))
        cerr << "[timing] startup seconds: until load " << (t_l0 - micros_start) * 1e-6 << "  index load " << (t_l1 - t_l0) * 1e-6 << "  upload + tables (first HIP call) "
             << (cur_time_micros() - t_l1) * 1e-6 << endl;
    (void)fin_set_option("pipeline_kmers", 1 << 24);   // three sub-batches per chunk: upload, search and download overlap inside a chunk too
    if (ngpus > 1) cerr << "Reads sharded by record over " << ngpus << " GPUs (index replicated)" << endl;
    cerr << "Index loaded" << endl;
    const int64_t k = index.get_k();
    cerr << "k = " << to_string(k) << " SBWT nodes: " << to_string(index.number_of_subsets()) << " kmers: " << to_string(index.number_of_kmers()) << endl;
    int64_t number_of_queries = 0;
    for (size_t i = 0; i < query_files.size(); i++) {
        write_log("Running streaming queries from input file " + query_files[i]);
        OutSink out(output_files.has_value() ? &output_files.value()[i] : nullptr);
        g_query_name = query_files[i];
        if (!g_paired && BlockReader::usable(query_files[i])) {   // (--paired 1: the record loop, which cuts chunks between fragments only)
            BlockReader breader(query_files[i]);
            number_of_queries += run_fmin_queries_streaming(nullptr, &breader, out, index, index_prefix + ".stats");
        } else {
            SeqReader reader(query_files[i]);
            number_of_queries += run_fmin_queries_streaming(&reader, nullptr, out, index, index_prefix + ".stats");
        }
    }
    if (g_seg_file) {
        const bool bad = fflush(g_seg_file) != 0 || ferror(g_seg_file);
        fclose(g_seg_file); g_seg_file = nullptr;
        if (bad) throw runtime_error("Error writing to file: " + seg_file);
    }
    if (g_rs_file) {
        const bool bad = fflush(g_rs_file) != 0 || ferror(g_rs_file);
        fclose(g_rs_file); g_rs_file = nullptr;
        if (bad) throw runtime_error("Error writing to file: " + rs_file);
    }
    if (g_scr_file) {
        const bool bad = fflush(g_scr_file) != 0 || ferror(g_scr_file);
        fclose(g_scr_file); g_scr_file = nullptr;
        if (bad) throw runtime_error("Error writing to file: " + scr_file);
    }
    if (g_cls_file) {
        const bool bad = fflush(g_cls_file) != 0 || ferror(g_cls_file);
        fclose(g_cls_file); g_cls_file = nullptr;
        if (bad) throw runtime_error("Error writing to file: " + cls_file);
    }
    if (g_tax_file) {
        const bool bad = fflush(g_tax_file) != 0 || ferror(g_tax_file);
        fclose(g_tax_file); g_tax_file = nullptr;
        if (bad) throw runtime_error("Error writing to file: " + taxa_file);
    }
    if (g_psa_file) {
        const bool bad = fflush(g_psa_file) != 0 || ferror(g_psa_file);
        fclose(g_psa_file); g_psa_file = nullptr;
        if (bad) throw runtime_error("Error writing to file: " + psa_file);
    }
    if (g_asg_file) {
        const bool bad = fflush(g_asg_file) != 0 || ferror(g_asg_file);
        fclose(g_asg_file); g_asg_file = nullptr;
        if (bad) throw runtime_error("Error writing to file: " + asg_file);
    }
    if (g_asg && !asg_report.empty()) {   // the counts of the run's assignment, kept on the device until now
        char err[512] = {0};
        const uint32_t nc = fin_colors_n_colors(g_colors);
        vector<uint64_t> assigned(nc), sole(nc);
        uint64_t counters[4] = {0, 0, 0, 0};
        if (fin_assign_download(g_asg, assigned.data(), sole.data(), counters, err, sizeof err) != FIN_OK) throw runtime_error(err);
        string text;
        for (uint32_t c = 0; c < nc; c++) { text += to_string(c); text += '\t'; text += to_string(assigned[c]); text += '\t'; text += to_string(sole[c]); text += '\n'; }
        text += "unaligned\t" + to_string(counters[1]) + "\nunassigned\t" + to_string(counters[2]) + "\nmulti\t" + to_string(counters[3]) + "\n";
        ofstream cf(asg_report, ios::binary | ios::trunc);
        cf.write(text.data(), (streamsize)text.size());
        if (!cf) throw runtime_error("Error writing to file: " + asg_report);
    }
    if (g_frag_file) {
        const bool bad = fflush(g_frag_file) != 0 || ferror(g_frag_file);
        fclose(g_frag_file); g_frag_file = nullptr;
        if (bad) throw runtime_error("Error writing to file: " + frag_file);
    }
    if (g_frag) {   // the run's fragment-length histogram: --fragment-lengths' file, and --ab-lengths' lengths in bases made effective lengths before the EM
        char err[512] = {0};
        vector<uint64_t> hist(frag_bins);
        uint64_t cnt[7] = {0, 0, 0, 0, 0, 0, 0};
        if (fin_fragments_download(g_frag, hist.data(), cnt, err, sizeof err) != FIN_OK) throw runtime_error(err);
        if (!fraglen_file.empty()) {
            string text;
            for (uint32_t b = 0; b < frag_bins; b++) {
                if (!hist[b]) continue;
                if (b == frag_bins - 1) text += ">=";
                text += to_string((uint64_t)b * frag_width); text += '\t'; text += to_string(hist[b]); text += '\n';
            }
            static const char* const names[6] = {"none", "one", "split", "tandem", "outward", "inward"};
            for (int c = 0; c < 6; c++) { text += names[c]; text += '\t'; text += to_string(cnt[c]); text += '\n'; }
            char num[64];
            if (cnt[FIN_FRAG_INWARD]) snprintf(num, sizeof num, "mean\t%.10g\n", (double)cnt[FIN_FRAG_LEN_SUM] / (double)cnt[FIN_FRAG_INWARD]);
            else snprintf(num, sizeof num, "mean\t-\n");
            text += num;
            ofstream cf(fraglen_file, ios::binary | ios::trunc);
            cf.write(text.data(), (streamsize)text.size());
            if (!cf) throw runtime_error("Error writing to file: " + fraglen_file);
        }
        if (ab_frag) {
            vector<uint64_t> ref(ab_lengths.size());
            for (size_t c = 0; c < ref.size(); c++) ref[c] = (uint64_t)ab_lengths[c];
            if (fin_effective_lengths(hist.data(), frag_bins, frag_width, ref.data(), ref.size(), ab_lengths.data()) != FIN_OK) throw runtime_error("--ab-fragment-lengths 1: fin_effective_lengths refused the histogram");
        }
    }
    if (g_eqc && !ab_file.empty()) {   // the abundances, estimated on the device from the run's classes: the rows stay there
        char err[512] = {0};
        const uint32_t nc = fin_colors_n_colors(g_colors);
        vector<double> alpha(nc);
        fin_abundance_info info;
        const double* const lens = ab_lengths.empty() ? nullptr : ab_lengths.data();
        vector<double> boot_mean, boot_sd;   // --ab-bootstraps: over the replicates, per colour
        if (ab_bootstraps) {
            const uint32_t B = ab_bootstraps;
            vector<double> boot((size_t)B * nc);
            vector<uint64_t> boot_reads(B);
            vector<uint32_t> boot_iters(B);
            vector<uint8_t> boot_conv(B);
            if (fin_eqclasses_bootstrap(g_eqc, lens, ab_max_iters, ab_tol, B, ab_seed, alpha.data(), &info, boot.data(), boot_reads.data(), boot_iters.data(), boot_conv.data(), err,
                                        sizeof err) != FIN_OK)
                throw runtime_error(err);
            boot_mean.assign(nc, 0.0); boot_sd.assign(nc, 0.0);
            for (uint32_t c = 0; c < nc; c++) {
                double sum = 0.0, dev = 0.0;
                for (uint32_t b = 0; b < B; b++) sum += boot[(size_t)b * nc + c];
                boot_mean[c] = sum / B;
                for (uint32_t b = 0; b < B; b++) dev += (boot[(size_t)b * nc + c] - boot_mean[c]) * (boot[(size_t)b * nc + c] - boot_mean[c]);
                boot_sd[c] = B > 1 ? std::sqrt(dev / (B - 1)) : 0.0;
            }
        } else if (fin_eqclasses_abundance(g_eqc, lens, ab_max_iters, ab_tol, alpha.data(), nullptr, &info, err, sizeof err) != FIN_OK)
            throw runtime_error(err);
        double per_len_sum = 0.0;
        for (uint32_t c = 0; c < nc; c++) per_len_sum += alpha[c] / (ab_lengths.empty() ? 1.0 : ab_lengths[c]);
        string text;
        char num[96];
        for (uint32_t c = 0; c < nc; c++) {
            const double share = per_len_sum > 0.0 ? alpha[c] / (ab_lengths.empty() ? 1.0 : ab_lengths[c]) / per_len_sum : 0.0;
            if (ab_bootstraps) snprintf(num, sizeof num, "%u\t%.10g\t%.10g\t%.10g\t%.10g\n", c, alpha[c], share, boot_mean[c], boot_sd[c]);
            else if (ab_frag) snprintf(num, sizeof num, "%u\t%.10g\t%.10g\t%.10g\n", c, alpha[c], share, ab_lengths[c]);   // (the effective lengths used)
            else snprintf(num, sizeof num, "%u\t%.10g\t%.10g\n", c, alpha[c], share);
            text += num;
        }
        text += "unaligned\t"; text += to_string(info.n_unaligned); text += '\n';
        text += "iterations\t"; text += to_string(info.iters); text += info.converged ? "\tconverged\n" : "\tmax_iters\n";
        snprintf(num, sizeof num, "loglik\t%.10g\n", info.loglik);
        text += num;
        if (ab_bootstraps) { text += "bootstraps\t"; text += to_string(ab_bootstraps); text += "\tseed\t"; text += to_string(ab_seed); text += '\n'; }
        ofstream cf(ab_file, ios::binary | ios::trunc);
        cf.write(text.data(), (streamsize)text.size());
        if (!cf) throw runtime_error("Error writing to file: " + ab_file);
    }
    if (g_eqc && (!eqc_file.empty() || !crep_file.empty())) {   // the classes and the tally derived from them, after the last chunk
        char err[512] = {0};
        const uint32_t W = fin_colors_words(g_colors), nc = fin_colors_n_colors(g_colors);
        uint64_t n = 0, un = 0;
        vector<uint64_t> rows(1), reads(1);
        int rc = fin_eqclasses_download(g_eqc, rows.data(), reads.data(), 0, &n, &un, err, sizeof err);   // (how many there are)
        if (rc == FIN_ELIMIT && n > 0) {
            rows.assign((size_t)n * W, 0); reads.assign((size_t)n, 0);
            rc = fin_eqclasses_download(g_eqc, rows.data(), reads.data(), n, &n, &un, err, sizeof err);
        }
        if (rc != FIN_OK) throw runtime_error(err);
        if (!eqc_file.empty()) {
            string text;
            for (uint64_t i = 0; i < n; i++) {
                uint32_t pc = 0;
                for (uint32_t w = 0; w < W; w++) pc += (uint32_t)__builtin_popcountll(rows[(size_t)i * W + w]);
                text += to_string(reads[(size_t)i]); text += '\t'; text += to_string(pc); text += '\t';
                append_colors(text, rows.data() + (size_t)i * W, W);
                text += '\n';
            }
            if (eqc_unaligned) { text += "unaligned\t"; text += to_string(un); text += '\n'; }
            ofstream cf(eqc_file, ios::binary | ios::trunc);
            cf.write(text.data(), (streamsize)text.size());
            if (!cf) throw runtime_error("Error writing to file: " + eqc_file);
        }
        if (!crep_file.empty()) {
            vector<uint64_t> with(nc), only(nc);
            if (fin_eqclasses_color_tally(rows.data(), reads.data(), n, nc, with.data(), only.data()) != FIN_OK) throw runtime_error("the colour tally of the equivalence classes failed");
            string text;
            for (uint32_t c = 0; c < nc; c++) { text += to_string(c); text += '\t'; text += to_string(with[c]); text += '\t'; text += to_string(only[c]); text += '\n'; }
            text += "unaligned\t"; text += to_string(un); text += '\n';
            ofstream cf(crep_file, ios::binary | ios::trunc);
            cf.write(text.data(), (streamsize)text.size());
            if (!cf) throw runtime_error("Error writing to file: " + crep_file);
        }
    }
    if (g_tax && g_tax_report) {   // the tally and the clade counts, after the last chunk: one line per taxon with a read at or below it, in the caller's ids
        char err[512] = {0};
        const size_t n = g_tax_ids.size();
        vector<uint64_t> direct(n + 1), clade(n);
        if (fin_taxonomy_download(g_tax, direct.data(), clade.data(), nullptr, err, sizeof err) != FIN_OK) throw runtime_error(err);
        string text;
        for (size_t t = 0; t < n; t++)
            if (clade[t]) { text += to_string(g_tax_ids[t]); text += '\t'; text += to_string(clade[t]); text += '\t'; text += to_string(direct[t]); text += '\n'; }
        text += "unclassified\t"; text += to_string(direct[n]); text += '\n';
        ofstream cf(taxrep_file, ios::binary | ios::trunc);
        cf.write(text.data(), (streamsize)text.size());
        if (!cf) throw runtime_error("Error writing to file: " + taxrep_file);
    }
    if (g_labels && g_cls_report) {   // the tally, after the last chunk: one line per label, then the unassigned reads
        char err[512] = {0};
        vector<uint64_t> reads((size_t)n_labels + 1);
        if (fin_labels_download(g_labels, reads.data(), nullptr, err, sizeof err) != FIN_OK) throw runtime_error(err);
        string text;
        for (size_t l = 0; l < n_labels; l++) { text += to_string(l); text += '\t'; text += to_string(reads[l]); text += '\n'; }
        text += "unassigned\t"; text += to_string(reads[n_labels]); text += '\n';
        ofstream cf(report_file, ios::binary | ios::trunc);
        cf.write(text.data(), (streamsize)text.size());
        if (!cf) throw runtime_error("Error writing to file: " + report_file);
    }
    if (!cover_file.empty()) {   // the coverage, after the last chunk: one line per unitig of the index
        char err[512] = {0};
        const size_t nu = (size_t)index.number_of_unitigs();
        vector<uint64_t> covered(nu + 1);
        vector<int64_t> ends(nu + 1);
        if (fin_cover_download(g_cover, nullptr, covered.data(), nullptr, err, sizeof err) != FIN_OK) throw runtime_error(err);
        if (fin_index_export(index.handle(), FIN_X_ENDS, ends.data(), nu * sizeof(int64_t), err, sizeof err) != FIN_OK) throw runtime_error(err);
        const int64_t k = index.get_k();
        string text;
        text.reserve(nu * 20);
        for (size_t u = 0; u < nu; u++) {
            const int64_t len = ends[u] - (u ? ends[u - 1] : 0);
            text += to_string(u); text += '\t'; text += to_string(len - k + 1); text += '\t'; text += to_string(covered[u]); text += '\n';
        }
        ofstream cf(cover_file, ios::binary | ios::trunc);
        cf.write(text.data(), (streamsize)text.size());
        if (!cf) throw runtime_error("Error writing to file: " + cover_file);
    }
    if (!depth_file.empty()) {   // the depth, after the last chunk: the prefix sum and the statistics on the device, one line per unitig of the index
        char err[512] = {0};
        const size_t nu = (size_t)index.number_of_unitigs();
        vector<fin_depth_stat> stats(nu + 1);
        vector<int64_t> ends(nu + 1);
        if (fin_depth_download(g_depth, min_depth, nullptr, stats.data(), nullptr, err, sizeof err) != FIN_OK) throw runtime_error(err);
        if (fin_index_export(index.handle(), FIN_X_ENDS, ends.data(), nu * sizeof(int64_t), err, sizeof err) != FIN_OK) throw runtime_error(err);
        const int64_t k = index.get_k();
        string text;
        text.reserve(nu * 32);
        for (size_t u = 0; u < nu; u++) {
            const int64_t len = ends[u] - (u ? ends[u - 1] : 0);
            text += to_string(u); text += '\t'; text += to_string(len - k + 1); text += '\t'; text += to_string(stats[u].sum); text += '\t';
            text += to_string(stats[u].max); text += '\t'; text += to_string(stats[u].n_at_least); text += '\n';
        }
        ofstream cf(depth_file, ios::binary | ios::trunc);
        cf.write(text.data(), (streamsize)text.size());
        if (!cf) throw runtime_error("Error writing to file: " + depth_file);
    }
    if (!links_file.empty()) {   // the links, after the last chunk: filtered, compacted and decoded on the device, in the canonical order
        char err[512] = {0};
        uint64_t n = 0, cnt[4] = {0, 0, 0, 0};
        if (fin_links_download(g_links, links_min_count, nullptr, 0, &n, cnt, err, sizeof err) != FIN_OK) throw runtime_error(string("--links (--max-links ") + to_string(max_links) + "): " + err);
        vector<fin_link> links((size_t)n + 1);
        if (fin_links_download(g_links, links_min_count, links.data(), n, &n, cnt, err, sizeof err) != FIN_OK) throw runtime_error(string("--links: ") + err);
        string text;
        text.reserve((size_t)n * 40 + 64);
        for (uint64_t i = 0; i < n; i++) {
            const fin_link& l = links[(size_t)i];
            text += to_string(l.u_a); text += '\t'; text += to_string(l.off_a); text += '\t'; text += to_string(l.u_b); text += '\t'; text += to_string(l.off_b); text += '\t';
            text += to_string(l.count); text += '\n';
        }
        text += "#transitions\t" + to_string(cnt[0]) + "\n#links\t" + to_string(cnt[1]) + "\n#self\t" + to_string(cnt[3]) + "\n";
        ofstream cf(links_file, ios::binary | ios::trunc);
        cf.write(text.data(), (streamsize)text.size());
        if (!cf) throw runtime_error("Error writing to file: " + links_file);
    }
    if (!colcov_file.empty()) {   // breadth and depth per reference, after the last chunk: projected on the device, one line per colour
        char err[512] = {0};
        const size_t nc = color_refs.size();
        vector<fin_color_coverage> cc(nc + 1);
        if (fin_colors_coverage(g_colors, g_cover, g_depth, min_depth, cc.data(), &cc[nc], err, sizeof err) != FIN_OK) throw runtime_error(err);
        string text;
        for (size_t c = 0; c < nc; c++) {
            const fin_color_coverage& e = cc[c];
            text += to_string(c);
            for (uint64_t v : {e.kmers, e.covered, e.kmers_only, e.covered_only, e.depth_sum, e.depth_sum_only, e.solid, e.solid_only}) { text += '\t'; text += to_string(v); }
            text += '\n';
        }
        text += "uncoloured";
        for (uint64_t v : {cc[nc].kmers, cc[nc].covered, cc[nc].depth_sum, cc[nc].solid}) { text += '\t'; text += to_string(v); }
        text += '\n';
        ofstream cf(colcov_file, ios::binary | ios::trunc);
        cf.write(text.data(), (streamsize)text.size());
        if (!cf) throw runtime_error("Error writing to file: " + colcov_file);
    }
    if (dh_asked) {   // the depth histograms, after the last chunk: binned on the device from the staged prefix sum
        char err[512] = {0};
        auto write_file = [](const string& name, const string& t) {
            ofstream cf(name, ios::binary | ios::trunc);
            cf.write(t.data(), (streamsize)t.size());
            if (!cf) throw runtime_error("Error writing to file: " + name);
        };
        // a bin's depth: its lower edge, the last of several bins as ">=X"
        auto bin_name = [&](uint32_t b) { return string(b == dh_bins - 1u && dh_bins > 1u ? ">=" : "") + to_string((uint64_t)b * dh_width); };
        if (!dh_file.empty()) {
            vector<uint64_t> hist(dh_bins);
            if (fin_depth_histogram(g_depth, dh_bins, dh_width, hist.data(), err, sizeof err) != FIN_OK) throw runtime_error(err);
            string text;
            for (uint32_t b = 0; b < dh_bins; b++) { text += bin_name(b); text += '\t'; text += to_string(hist[b]); text += '\n'; }
            write_file(dh_file, text);
        }
        if (!cdh_file.empty() || !cdq_file.empty()) {
            const size_t nc = color_refs.size();
            vector<uint64_t> tab(nc * 2 * dh_bins), unc(dh_bins);
            if (fin_colors_depth_histogram(g_colors, g_depth, dh_bins, dh_width, tab.data(), unc.data(), err, sizeof err) != FIN_OK) throw runtime_error(err);
            if (!cdh_file.empty()) {   // the non-zero entries
                string text;
                for (size_t c = 0; c < nc; c++)
                    for (int j = 0; j < 2; j++)
                        for (uint32_t b = 0; b < dh_bins; b++)
                            if (const uint64_t v = tab[(c * 2 + j) * dh_bins + b]) { text += to_string(c); text += j ? "\tonly\t" : "\tall\t"; text += bin_name(b); text += '\t'; text += to_string(v); text += '\n'; }
                for (uint32_t b = 0; b < dh_bins; b++)
                    if (unc[b]) { text += "uncoloured\t-\t"; text += bin_name(b); text += '\t'; text += to_string(unc[b]); text += '\n'; }
                write_file(cdh_file, text);
            }
            if (!cdq_file.empty()) {
                // the quantile rule of finito_amd.h: t = max(1, ceil(p N / 1000)), the smallest bin whose cumulative count reaches t; "-" without k-mers.  (N is
                // below 2^32, the text's length: p N fits 64 bits)
                auto quantile = [&](const uint64_t* h, uint64_t N, uint32_t p) -> string {
                    if (N == 0) return "-";
                    const uint64_t t = max<uint64_t>(1, ((uint64_t)p * N + 999u) / 1000u);
                    uint64_t acc = 0;
                    for (uint32_t b = 0; b < dh_bins; b++) { acc += h[b]; if (acc >= t) return bin_name(b); }
                    return "-";   // (not reached: t <= N)
                };
                string text;
                for (size_t c = 0; c < nc; c++) {
                    text += to_string(c);
                    for (int j = 0; j < 2; j++) {
                        const uint64_t* h = tab.data() + (c * 2 + j) * dh_bins;
                        uint64_t N = 0;
                        for (uint32_t b = 0; b < dh_bins; b++) N += h[b];
                        text += '\t'; text += to_string(N);
                        for (uint32_t p : {250u, 500u, 750u}) { text += '\t'; text += quantile(h, N, p); }
                    }
                    text += '\n';
                }
                write_file(cdq_file, text);
            }
        }
    }
    if (!colsim_cov_file.empty()) write_color_similarity(colsim_cov_file, g_cover, color_refs.size());   // ... and in what the run found, after the last chunk
    if (g_pileup) {   // the pileup, after the last chunk: the covered positions, and the candidates called on the device
        char err[512] = {0};
        const size_t nu = (size_t)index.number_of_unitigs();
        uint64_t counters[4] = {0, 0, 0, 0};
        auto line = [](string& t, uint64_t u, uint64_t off, uint32_t ref, uint32_t cover, const uint32_t* alt) {
            t += to_string(u); t += '\t'; t += to_string(off); t += '\t'; t += "ACGT"[ref & 3u]; t += '\t'; t += to_string(cover);
            for (int b = 0; b < 4; b++) { t += '\t'; t += to_string(alt[b]); }
            t += '\n';
        };
        auto last_line = [&](string& t) {
            t += "#reads";
            for (int c = 0; c < 4; c++) { t += '\t'; t += to_string(counters[c]); }
            t += '\n';
        };
        auto write_file = [](const string& name, const string& t) {
            ofstream cf(name, ios::binary | ios::trunc);
            cf.write(t.data(), (streamsize)t.size());
            if (!cf) throw runtime_error("Error writing to file: " + name);
        };
        if (!pileup_file.empty()) {
            const size_t total = (size_t)fin_index_total_len(index.handle());
            vector<uint32_t> cover(total + 1), alt(4 * total + 4);
            vector<uint8_t> concat(total + 1);
            vector<int64_t> ends(nu + 1);
            if (fin_pileup_download(g_pileup, cover.data(), alt.data(), counters, err, sizeof err) != FIN_OK) throw runtime_error(err);
            if (fin_index_export(index.handle(), FIN_X_ENDS, ends.data(), nu * sizeof(int64_t), err, sizeof err) != FIN_OK) throw runtime_error(err);
            if (fin_index_export(index.handle(), FIN_X_CONCAT, concat.data(), total, err, sizeof err) != FIN_OK) throw runtime_error(err);
            string text;
            for (size_t u = 0; u < nu; u++) {
                const size_t start = u ? (size_t)ends[u - 1] : 0;
                for (size_t g = start; g < (size_t)ends[u]; g++) if (cover[g]) line(text, u, g - start, concat[g], cover[g], &alt[4 * g]);
            }
            last_line(text);
            write_file(pileup_file, text);
        }
        if (!variants_file.empty()) {
            if (fin_pileup_download(g_pileup, nullptr, nullptr, counters, err, sizeof err) != FIN_OK) throw runtime_error(err);
            vector<fin_variant> v(1024);
            uint64_t n = 0;
            for (;;) {   // a call that does not fit says how many there are
                const int rc = fin_pileup_call(g_pileup, min_alt, min_alt_permille, v.data(), v.size(), &n, err, sizeof err);
                if (rc == FIN_OK) break;
                if (rc != FIN_ELIMIT || n <= v.size()) throw runtime_error(err);
                v.resize((size_t)n);
            }
            string text;
            for (uint64_t q = 0; q < n; q++) line(text, v[q].u, v[q].off, v[q].ref, v[q].cover, v[q].alt);
            last_line(text);
            write_file(variants_file, text);
        }
    }
    if (!refdepth_file.empty()) {   // the depth along every reference record, lifted on the device after the last chunk
        char err[512] = {0};
        const size_t ns = ref_ids.size();
        vector<uint32_t> nk(ns + 1);
        vector<uint64_t> wo(ns + 1, 0);
        if (fin_refpaths_download(g_refpaths, nk.data(), nullptr, nullptr, err, sizeof err) != FIN_OK) throw runtime_error(err);
        vector<fin_ref_window> win(1);
        uint64_t n = 0;
        for (;;) {   // a call that does not fit says how many there are
            const int rc = fin_refpaths_depth(g_refpaths, g_depth, ref_window, min_depth, wo.data(), win.data(), win.size(), &n, err, sizeof err);
            if (rc == FIN_OK) break;
            if (rc != FIN_ELIMIT || n <= win.size()) throw runtime_error(err);
            win.resize((size_t)n);
        }
        ofstream cf(refdepth_file, ios::binary | ios::trunc);
        string text;
        for (size_t s = 0; s < ns; s++) {
            for (uint64_t w = wo[s]; w < wo[s + 1]; w++) {
                const uint64_t start = (w - wo[s]) * ref_window, end = min<uint64_t>(nk[s], start + ref_window);
                text += to_string(ref_ids[s].first); text += '\t'; text += to_string(ref_ids[s].second); text += '\t'; text += to_string(start); text += '\t';
                text += to_string(end); text += '\t'; text += to_string(win[w].in_graph); text += '\t'; text += to_string(win[w].covered); text += '\t';
                text += to_string(win[w].depth_sum); text += '\n';
            }
            if (text.size() >= (8u << 20)) { cf.write(text.data(), (streamsize)text.size()); text.clear(); }
        }
        cf.write(text.data(), (streamsize)text.size());
        if (!cf) throw runtime_error("Error writing to file: " + refdepth_file);
    }
    if (!refvar_file.empty()) {   // the pileup's candidates under every reference record that crosses them
        char err[512] = {0};
        vector<fin_variant> v(1024);
        uint64_t n = 0;
        for (;;) {
            const int rc = fin_pileup_call(g_pileup, min_alt, min_alt_permille, v.data(), v.size(), &n, err, sizeof err);
            if (rc == FIN_OK) break;
            if (rc != FIN_ELIMIT || n <= v.size()) throw runtime_error(err);
            v.resize((size_t)n);
        }
        vector<fin_ref_variant> lifted((size_t)(4 * n + 1024));
        uint64_t m = 0;
        for (;;) {
            const int rc = fin_refpaths_lift_variants(g_refpaths, v.data(), n, lifted.data(), lifted.size(), &m, err, sizeof err);
            if (rc == FIN_OK) break;
            if (rc != FIN_ELIMIT || m <= lifted.size()) throw runtime_error(err);
            lifted.resize((size_t)m);
        }
        string text;
        for (uint64_t q = 0; q < m; q++) {
            const fin_ref_variant& l = lifted[q];
            const fin_variant& x = v[l.var];
            const bool rev = l.flags & 1u;
            text += to_string(ref_ids[l.seq].first); text += '\t'; text += to_string(ref_ids[l.seq].second); text += '\t'; text += to_string((uint64_t)l.pos + 1); text += '\t';
            text += rev ? '-' : '+'; text += '\t'; text += "ACGT"[(rev ? 3u - x.ref : x.ref) & 3u]; text += '\t'; text += to_string(x.cover);
            for (int b = 0; b < 4; b++) { text += '\t'; text += to_string(x.alt[rev ? 3 - b : b]); }
            text += '\t'; text += to_string(x.u); text += '\t'; text += to_string(x.off); text += '\n';
        }
        ofstream cf(refvar_file, ios::binary | ios::trunc);
        cf.write(text.data(), (streamsize)text.size());
        if (!cf) throw runtime_error("Error writing to file: " + refvar_file);
    }
    if (g_hits && !counts_file.empty()) {   // the profile, after the last chunk: one line per unitig of the index
        char err[512] = {0};
        vector<uint64_t> counts((size_t)index.number_of_unitigs() + 1);
        if (fin_hits_download(g_hits, counts.data(), nullptr, err, sizeof err) != FIN_OK) throw runtime_error(err);
        string text;
        text.reserve(counts.size() * 12);
        for (size_t u = 0; u + 1 < counts.size(); u++) { text += to_string(u); text += '\t'; text += to_string(counts[u]); text += '\n'; }
        ofstream cf(counts_file, ios::binary | ios::trunc);
        cf.write(text.data(), (streamsize)text.size());
        if (!cf) throw runtime_error("Error writing to file: " + counts_file);
    }
    prewarm_stop = true;
    if (prewarm.joinable()) prewarm.join();
    for (fin_text* t : g_prewarmed.texts) fin_text_free(t);
    for (auto& b : g_prewarmed.bases) fin_host_free(b.first);
    g_prewarmed.texts.clear(); g_prewarmed.bases.clear();
    int64_t new_total_micros = cur_time_micros() - micros_start;
    write_log("us/query end-to-end: " + to_string((double)new_total_micros / (double)number_of_queries));
    write_log("total number of queries: " + to_string(number_of_queries));
    ofstream statsfile2(index_prefix + "stats.txt", ios::app);   // sic: no dot, search_fmin.hh:197
    statsfile2 << "," + to_string((double)new_total_micros / (double)number_of_queries);
    int64_t bytes = index.size_in_bytes();
    write_log("bytes: " + to_string(bytes));
    {   // (the reference's two figures are the INDEX's -- size_in_bytes(), FinimizerIndex.hh:244-258 -- and stay so in the stats file;
        //  what a replica of it occupies in HBM with every table the upload derives is logged beside them)
        const int64_t tables = index.replica_table_bytes();
        if (tables >= 0) {
            write_log("bytes in HBM per replica (index + derived tables): " + to_string(bytes + tables));
            write_log("bits per k-mer in HBM per replica: " + to_string(static_cast<double>((bytes + tables) * 8) / (double)index.number_of_kmers()));
        }
    }
    statsfile2 << "," + to_string(bytes);
    statsfile2 << "," + to_string(static_cast<double>(bytes * 8) / (double)index.number_of_kmers()) + "\n";
    statsfile2 << "," + to_string(index.number_of_kmers()) + "\n";
    return 0;
}

// diagnostic (not a reference command): the reads a file yields, one per line -- `finito parse-reads <file> [seq|block] [block bytes]`;
// tests compare the block-parallel reader with the sequential one on irregular files
static int parse_reads(int argc, char** argv) {
    if (argc < 2) { cerr << "usage: parse-reads <file> [seq|block] [block bytes]" << endl; return 1; }
    const string path = argv[1], which = argc > 2 ? argv[2] : "block";
    const size_t block = argc > 3 ? (size_t)stoull(argv[3]) : (256u << 20);
    if (which == "seq" || !BlockReader::usable(path)) {
        SeqReader r(path);
        while (r.get_next_read_to_buffer() > 0) { fwrite(r.read_buf.data(), 1, r.read_buf.size(), stdout); fputc('\n', stdout); }
    } else {
        BlockReader r(path);
        vector<char> dst; size_t nb = 0; vector<uint64_t> offs;
        const bool quiet = getenv("FINITO_PARSE_QUIET") != nullptr;   // timing only
        const int64_t t0 = cur_time_micros(); uint64_t n_reads = 0, n_bases = 0;
        while (r.next(block, [&](size_t n) { if (dst.size() < n) dst.resize(n); return dst.data(); }, nb, offs)) {
            n_reads += offs.size() - 1; n_bases += nb;
            if (!quiet) for (size_t i = 0; i + 1 < offs.size(); i++) { fwrite(dst.data() + offs[i], 1, (size_t)(offs[i + 1] - offs[i]), stdout); fputc('\n', stdout); }
        }
        if (quiet) cerr << n_reads << " reads, " << n_bases << " bases in " << (cur_time_micros() - t0) * 1e-6 << " s" << endl;
    }
    return 0;
}

static vector<string> commands = {"build-fmin", "search-fmin"};
static void print_help(char** argv) {
    cerr << "Available commands: " << endl;
    for (auto& S : commands) cerr << "   " << argv[0] << " " << S << endl;
    cerr << "Running a command without arguments prints the usage instructions for the command." << endl;
}

int main(int argc, char** argv) {
    omp_set_num_threads(fin_host_threads());
    if (argc == 1) { print_help(argv); return 1; }
    string command = argv[1];
    if (command == "--help" || command == "-h") { print_help(argv); return 1; }
    for (int i = 1; i < argc; i++) argv[i - 1] = argv[i];
    argc--;
    try {
        if (command == "build-fmin") return build_fmin(argc, argv);
        else if (command == "search-fmin") return search_fmin(argc, argv);
        else if (command == "parse-reads") return parse_reads(argc, argv);
        else throw runtime_error("Invalid command: " + command);
    } catch (const runtime_error& e) {
        cerr << "Runtime error: " << e.what() << '\n';
        return 1;
    } catch (const exception& e) {
        cerr << "Error: " << e.what() << '\n';
        return 1;
    }
}
