"""Shared helpers for the tests (small pure-numpy synthetic inputs; the big seeded generator is finito_amd.synth)."""
import numpy as np

_RC = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s[::-1].translate(_RC)


def random_genome(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, n))


def cut_unitigs(rng, genome, k, max_len=200, flip=True, shuffle=True):
    """Pieces overlapping by k-1 (every genome k-mer in exactly one piece), randomly reverse-complemented."""
    pieces, s, n = [], 0, len(genome)
    while s + k <= n:
        L = int(rng.integers(k, max_len + 1))
        e = min(n, s + L)
        if n - e < 1:
            e = n
        pieces.append(genome[s:e])
        if e == n:
            break
        s = e - (k - 1)
    if flip:
        pieces = [p if rng.random() < 0.5 else rc(p) for p in pieces]
    if shuffle:
        order = rng.permutation(len(pieces))
        pieces = [pieces[i] for i in order]
    return pieces


def sample_reads(rng, genome, n_reads, read_len, err=0.01, random_frac=0.05):
    reads = []
    n = len(genome)
    for _ in range(n_reads):
        if rng.random() < random_frac:
            reads.append(random_genome(rng, read_len))
            continue
        a = int(rng.integers(0, n - read_len + 1))
        r = list(genome[a:a + read_len])
        for i in range(read_len):
            if rng.random() < err:
                r[i] = "ACGT"[(("ACGT".index(r[i])) + int(rng.integers(1, 4))) % 4]
        r = "".join(r)
        reads.append(r if rng.random() < 0.5 else rc(r))
    return reads


# ---- the chunk format of a step, restated without the package ------------------------------------------------------------------------
# A chunk = 32 bases of one strand as {u64 2-bit codes (A0 C1 G2 T3, base j at bits 2j), u32 validity bits, u32 0}; per read
# [forward chunks | reverse-complement chunks], ceil(len / 32) of each.  A byte is a base iff b & 0xDF is one of "ACGT" (the reference's
# c & ~32, common.hh:106); any other byte, and every position past the read, has code 0 and validity bit 0.  The reverse strand's
# position i is the complement (3 - code) of byte len-1-i, where that byte is a base.
_REF_CODE = np.zeros(256, dtype=np.uint64)
_REF_VALID = np.zeros(256, dtype=bool)
for _b in range(256):
    if (_b & 0xDF) in b"ACGT":
        _REF_CODE[_b] = b"ACGT".index(_b & 0xDF)
        _REF_VALID[_b] = True


def ref_chunks(reads):
    """the packed chunks of a read set as the format states them: uint32 [n_chunks, 4] (lo codes, hi codes, validity, 0)"""
    codes, valid = [], []
    for s in reads:
        a = np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), dtype=np.uint8)
        n = len(a)
        width = 32 * ((n + 31) // 32)
        for strand in (a, a[::-1]):
            c = np.zeros(width, dtype=np.uint64)
            v = np.zeros(width, dtype=bool)
            v[:n] = _REF_VALID[strand]
            c[:n] = _REF_CODE[strand]
            if strand is not a:
                c[:n] = np.where(v[:n], 3 - c[:n], 0)
            codes.append(c)
            valid.append(v)
    if not codes:
        return np.zeros((0, 4), dtype=np.uint32)
    c = np.concatenate(codes).reshape(-1, 32)
    v = np.concatenate(valid).reshape(-1, 32)
    sh = np.arange(32, dtype=np.uint64)
    w = (c << (2 * sh)).sum(axis=1, dtype=np.uint64)
    m = (v.astype(np.uint64) << sh).sum(axis=1, dtype=np.uint64)
    out = np.zeros((len(w), 4), dtype=np.uint32)
    out[:, 0] = (w & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    out[:, 1] = (w >> np.uint64(32)).astype(np.uint32)
    out[:, 2] = m.astype(np.uint32)
    return out


def chunk_offsets(reads):
    """first chunk of every read, and the total at the end: int64 [n_reads + 1]"""
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([2 * ((len(r) + 31) // 32) for r in reads])
    return off


def unpack_bits(words, n):
    return np.unpackbits(np.ascontiguousarray(words, dtype=np.uint64).view(np.uint8), bitorder="little")[:n]


def mosaic_read(rng, g, k, max_len):
    """pieces of the genome (either strand) with substitutions at a per-read rate, junk in between, the odd non-ACGT base"""
    out = []
    err = [0.0, 0.0, 0.005, 0.02, 0.1][int(rng.integers(0, 5))]
    L = int(rng.integers(0, max_len))
    while sum(len(x) for x in out) < L:
        t = int(rng.integers(0, 10))
        if t < 7:
            a = int(rng.integers(0, len(g) - 1)); n = int(rng.integers(1, max(2, min(L + 1, 6 * k))))
            piece = g[a:a + n]
            if rng.random() < 0.5:
                piece = rc(piece)
            piece = list(piece)
            for i in range(len(piece)):
                if rng.random() < err:
                    piece[i] = "ACGT"[int(rng.integers(0, 4))]
            out.append("".join(piece))
        elif t < 9:
            out.append(random_genome(rng, int(rng.integers(1, 3 * k))))
        else:
            out.append("N" if rng.random() < 0.7 else "n")
    return "".join(out)[:L]


# ---- the deferred second strand's hard family -------------------------------------------------------------------------
# The reference's forward walk (FinimizerIndex.hh:47-102) compares ONE new base per step with the unitig text behind its anchor; with
# duplicated unitigs the branch dictionary's rank names the wrong copy (common.hh:61-67) and the walk follows a text that does not spell
# the read's k-mers -- into slots where the reverse strand found the true place; the forward pair wins the merge (search_fmin.hh:54-60).
DEFER_KAT = [   # (k, unitigs, read): the judge's three minimised counter-examples of round 3's CPU restatement (faithful pair of the last slot)
    (12, ["AAAGGACCGGACTTG", "GACAAGTCCGGTC", "GACTTTTCCCGG", "GACTTTTCCCGG", "CCCAGAGACGGTTC"], "GGACAAGTCCGGTCC", (3, 2)),
    (21, ["CGTGACCCATTATTATCTCGCAAGTGGTTAAAAACGCGCGGTCGGCCCTAGTTAAGGCGGCTCGGCGTTTAGTC",
          "GTGACCCATTATTATCTCGCAAGTGGTTAAAAACGCGCGGTCGGCCCTAGTTAAGGCGGCTCGGCGTTTAA", "GGTTGCTGATTAAACGCCGAGCCGCCTT"],
     "TCCCATTATTATCTCGCAAGTGGTTAAAAACGCGCGGTCGGCCCTAGTTAAGGCGGCTCGGCGTTTAATC", (1, 53)),
    (31, ["CCACTACAGTCCTCAAACTGAGGACTGCAAGAACCCAATTCA", "GTATTGATACTAGAGATGATTGAGAGTAAAGCCTCTTCGACCC", "GCCTAGCTTCTTGTTTGCACTCTCATTTCAC",
          "GCCTAGCTTCTTGTTTGCACTCTCATTTCAC", "TGTACCATTTCGACAGAGGGTGTGTGAATTGGGTTCTTGCAGTCCTCAGTTTGA"],
     "TCCACTACAGTCCTCAAACTGAGGACTGCAAGAACCCAATTCAC", (2, 12)),
]


def defer_family_case(rng, case, k, n_reads=60):
    """One index set + reads of the family on which a deferred strand's walk matters: identical unitigs, near-duplicates that differ in their
    last (or first) bases, reverse-complement copies, duplicated stretches; reads = mosaics and samples AND their reverse complements, the
    unitigs and their reverse complements themselves, reads that run one or a few bases past a unitig's end (either end, either strand).
    Returns (genome, unitigs, reads)."""
    from tests.test_oracle_lazy import non_disjoint_sets
    fam = case % 5
    if fam == 0:
        g, unitigs = non_disjoint_sets(rng, int(rng.integers(0, 4)), k)
    else:
        g = random_genome(rng, int(rng.integers(6 * k + 50, 40 * k + 400)))
        if fam >= 3:   # duplicated stretches inside the genome
            for _ in range(int(rng.integers(1, 4))):
                a = int(rng.integers(0, max(1, len(g) - 3 * k))); n = int(rng.integers(k + 1, 5 * k)); at = int(rng.integers(0, len(g)))
                g = g[:at] + g[a:a + n] + g[at:]
        unitigs = cut_unitigs(rng, g, k, max_len=int(rng.integers(k + 2, 6 * k + 40)), flip=bool(case & 1))
    unitigs = [u for u in unitigs if len(u) >= k]
    base = list(unitigs)
    for _ in range(int(rng.integers(1, 5))):          # identical copies
        unitigs.insert(int(rng.integers(0, len(unitigs) + 1)), base[int(rng.integers(0, len(base)))])
    for _ in range(int(rng.integers(1, 5))):          # near-duplicates: last / first bases changed, cut or grown
        u = base[int(rng.integers(0, len(base)))]
        t = int(rng.integers(0, 4)); m = int(rng.integers(1, 4))
        if t == 0: v = u[:-m] + random_genome(rng, m)
        elif t == 1: v = random_genome(rng, m) + u[m:]
        elif t == 2: v = u + random_genome(rng, m)
        else: v = u[:max(k, len(u) - m)]
        if len(v) >= k:
            unitigs.insert(int(rng.integers(0, len(unitigs) + 1)), v)
    for _ in range(int(rng.integers(0, 4))):          # reverse-complement copies (whole or part)
        u = base[int(rng.integers(0, len(base)))]
        a = int(rng.integers(0, len(u) - k + 1))
        unitigs.insert(int(rng.integers(0, len(unitigs) + 1)), rc(u[a:a + int(rng.integers(k, len(u) - a + 1))]))
    L = min(len(g), int(rng.integers(k, 6 * k + 60)))
    reads = [mosaic_read(rng, g, k, 5 * k + 100) for _ in range(n_reads // 3)]
    reads += sample_reads(rng, g, n_reads // 3, L, err=float(rng.choice([0.0, 0.0, 0.01, 0.03])), random_frac=0.03)
    for u in unitigs[:40]:                             # the unitigs themselves, and reads that run past their ends
        reads.append(u)
        for _ in range(2):
            t = int(rng.integers(0, 5)); m = int(rng.integers(1, 4)); j = random_genome(rng, m)
            if t == 0: reads.append(u + j)
            elif t == 1: reads.append(j + u)
            elif t == 2: reads.append(j + u + random_genome(rng, 1))
            elif t == 3 and len(u) > k + 2:
                a = int(rng.integers(0, len(u) - k)); reads.append(u[a:] + j)
            else:
                w = list(u); w[int(rng.integers(0, len(w)))] = "ACGTN"[int(rng.integers(0, 5))]; reads.append("".join(w))
    reads += [rc(r) for r in reads]
    return g, unitigs, reads


# ---- hand-made fast-path records (include/finito_amd.h: fin_read_record; fin_batch_set_records) ---------------------------------------
# The pair pre-pass writes records with at most four positions for reads of at most 256 bases; the format -- and every device consumer of it -- allows eight
# positions and nk up to 2^16 - 1.  This generator makes the whole format: all three kinds mixed inside every wave of 64 reads, three blocks of 256 reads of one
# kind each (the kind-1 block on ONE unitig), 0 to 8 positions on either strand drawn from the shapes in _record_positions.  Kind-1 records and kind-0 pairs
# name real places of the unitig set (`ends`), so bitmap, depth and text of the result mean something.
UNIFORM_BLOCKS = ((3, 1), (6, 0), (9, 2))   # (block of 256 reads, its kind)
POSITION_SHAPES = 7


def _record_positions(rng, nk, k, nE, shape):
    """nE ascending positions in [0, nk + k - 2]: 0 uniform; 1 clustered, neighbours 0..k apart (gaps that overlap, touch at exactly k, coincide); 2 equal
    neighbours; 3 all below k - 1 (a gap clamped at slot 0); 4 all at or above nk (clamped at nk - 1); 5 drawn from k - 1, nk - 1, nk, nk + k - 2;
    6 a set that covers every slot (where nE * k >= nk, else uniform)"""
    top = nk + k - 2
    if nE == 0:
        return []
    if shape == 6 and nE * k < nk:
        shape = 0
    if shape == 0:
        E = rng.integers(0, top + 1, nE)
    elif shape == 1:
        E = int(rng.integers(0, top + 1)) + np.concatenate([[0], np.cumsum(rng.integers(0, k + 1, nE - 1))])
    elif shape == 2:
        E = np.repeat(rng.integers(0, top + 1, (nE + 1) // 2), 2)[:nE]
    elif shape == 3:
        E = rng.integers(0, k - 1, nE)
    elif shape == 4:
        E = rng.integers(nk, top + 1, nE)
    elif shape == 5:
        E = rng.choice([k - 1, nk - 1, nk, top], nE)
    else:
        E = (np.arange(nE) + 1) * k - 1
    return sorted(int(min(x, top)) for x in E)


def hand_made_record(rng, rec, nk, k, kmers, nE, rev, shape, u=None):
    """fill `rec` (one element of a RECORD_DTYPE array) as a kind-1 record of nk slots inside a unitig with room for them (kmers[u] = its number of k-mers):
    off0 = 0, off0 such that the last slot is the unitig's last k-mer, or anything between"""
    if u is None:
        ok = np.nonzero(kmers >= nk)[0]
        u = int(ok[rng.integers(0, len(ok))])
    room = int(kmers[u]) - nk
    assert room >= 0
    t = rng.random()
    Es = _record_positions(rng, nk, k, nE, shape)
    rec["u"], rec["off0"], rec["nk"] = u, 0 if t < 0.25 else room if t < 0.5 else int(rng.integers(0, room + 1)), nk
    rec["meta"] = nE | (rev << 8) | (1 << 16)
    rec["Es"] = sum(E << (16 * e) for e, E in enumerate(Es[:4])); rec["Es2"] = sum(E << (16 * e) for e, E in enumerate(Es[4:]))


def searched_read_pairs(rng, nk, kmers):
    """a kind-0 read's pairs: ascending and descending runs inside a unitig, absent stretches, one pair repeated"""
    out = []
    while len(out) < nk:
        n = min(nk - len(out), int(rng.integers(1, 90)))
        t = rng.random()
        if t < 0.2:
            out += [(-1, -1)] * n
            continue
        u = int(rng.integers(0, len(kmers))); n = min(n, int(kmers[u])); a = int(rng.integers(0, int(kmers[u]) - n + 1))
        out += [(u, a)] * n if t < 0.3 else [(u, o) for o in (range(a, a + n) if t < 0.65 else range(a + n - 1, a - 1, -1))]
    return out


def hand_made_records(rng, nks, k, ends):
    """(recs RECORD_DTYPE[len(nks)], int32 stream [n, 2]) in the form fin_batch_download_records delivers: a kind-0 record is {0, 0, 0, nk, 0, 0} and its pairs
    are the next nk of the stream.  nks[r] >= 1 is read r's number of k-mers; ends = the unitigs' cumulative ends (FIN_X_ENDS)"""
    import finito_amd as fa
    nks = np.asarray(nks, dtype=np.int64); n = len(nks)
    ends = np.asarray(ends, dtype=np.int64)
    kmers = np.diff(np.concatenate([[0], ends])) - k + 1
    assert (nks >= 1).all() and (kmers >= 1).all() and nks.max() <= kmers.max() and n >= 256 * (UNIFORM_BLOCKS[-1][0] + 1)
    kinds = rng.choice(3, n, p=[0.14, 0.74, 0.12])
    for w in range(0, n - 2, 64):                       # every wave holds all three kinds
        kinds[w + rng.permutation(min(64, n - w))[:3]] = [0, 1, 2]
    for blk, kind in UNIFORM_BLOCKS:
        kinds[256 * blk:256 * blk + 256] = kind
    ones = np.nonzero(kinds == 1)[0]
    cell = rng.permutation(len(ones)) % 18              # nE uniform over 0..8 on either strand, every combination equally often
    one_unitig = int(np.argmax(kmers))
    in_block = {r for blk, kind in UNIFORM_BLOCKS if kind == 1 for r in range(256 * blk, 256 * blk + 256)}
    recs = np.zeros(n, dtype=fa.RECORD_DTYPE)
    recs["nk"] = nks
    recs["meta"][kinds == 2] = 2 << 16
    stream = []
    for r in np.nonzero(kinds == 0)[0]:
        stream += searched_read_pairs(rng, int(nks[r]), kmers)
    for j, r in enumerate(ones):
        hand_made_record(rng, recs[r:r + 1], int(nks[r]), k, kmers, int(cell[j] % 9), int(cell[j] // 9), int(rng.integers(0, POSITION_SHAPES)),
                         u=one_unitig if int(r) in in_block else None)
    return recs, np.array(stream, dtype=np.int32).reshape(-1, 2)


_HAND_MADE = {}


def hand_made_case(k):
    """the one input the device consumers (tests/test_records_device.py) and the host functions (tests/test_records_host.py) both face at this k: a 40 000-base
    genome cut into unitigs of at most 700 bases, 3 019 reads of k .. 300 bases whose content is free (they fix nk), hand-made records over them, and
    `pairs` = what the records mean (tests/test_records.py::brute_expand).  Made once per k and shared; nobody changes it"""
    if k not in _HAND_MADE:
        from types import SimpleNamespace
        from oracle.oracle import OracleIndex
        from tests.test_records import brute_expand
        rng = np.random.default_rng(5000 + k)
        g = random_genome(rng, 40000)
        unitigs = cut_unitigs(rng, g, k, max_len=700)
        ends = OracleIndex.build(unitigs, k).ends()
        lens = rng.integers(k, 301, 3019)
        bases = rng.integers(0, 4, int(lens.sum()))
        reads, at = [], 0
        for L in lens:
            reads.append("".join("ACGT"[x] for x in bases[at:at + L])); at += int(L)
        nks = lens - k + 1
        recs, stream = hand_made_records(rng, nks, k, ends)
        pairs = brute_expand(recs, stream, k)
        for a in (ends, nks, recs, stream, pairs):
            a.setflags(write=False)
        _HAND_MADE[k] = SimpleNamespace(k=k, genome=g, unitigs=unitigs, ends=ends, reads=reads, nks=nks, recs=recs, stream=stream, pairs=pairs)
    return _HAND_MADE[k]


# ---- the tables an upload derives on the device, restated from their definitions (finito_amd/csrc/fin_format.h: FinDevIndex) ---------------------------
# Inputs are what fin_index_export gives -- the text as one code per base (FIN_X_CONCAT), the unitigs' exclusive ends (FIN_X_ENDS), the C array and the four
# planes as one 0/1 per node -- and, for the safe places, the oracle.  Nothing here calls the library.
FIN_CBF_BITS = 5
_M64 = (1 << 64) - 1


def text_of(concat):
    return "".join("ACGT"[c] for c in concat)


def default_cbf_m(k):
    """the string length an upload picks for its string filters by itself: 20, less for k < 29 (3 (k - m + 1) >= k)"""
    return max(1, min(k + 1 - (k + 2) // 3, 20, k))


def string_key(s):
    """key of a string: sum code(s[j]) << 2j"""
    return sum("ACGT".index(ch) << (2 * j) for j, ch in enumerate(s))


def cbf_hash(key):
    """fin_cbf_hash on a Python integer"""
    key ^= key >> 29; key = (key * 0xBF58476D1CE4E5B9) & _M64; key ^= key >> 32; key = (key * 0x94D049BB133111EB) & _M64; key ^= key >> 29
    return key


def cbf_bits(key, log2):
    """the bit numbers (in the whole filter) a string with this key sets / needs: FIN_CBF_BITS of them inside one block of 128"""
    h = cbf_hash(key)
    block = (h >> 35) & ((1 << log2) - 1)
    return [128 * block + ((h >> (7 * i)) & 127) for i in range(FIN_CBF_BITS)]


def string_keys(concat, ends, m):
    """every string of m bases that lies inside one unitig: (its key, its reverse complement's key, the text position of its last base), uint64 / int64 arrays"""
    code = np.asarray(concat, dtype=np.uint64)
    n = len(code)
    if n < m:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int64)
    uid = np.searchsorted(np.asarray(ends, dtype=np.int64), np.arange(n), side="right")
    a = np.nonzero(uid[:n - m + 1] == uid[m - 1:])[0]
    f = np.zeros(len(a), dtype=np.uint64); v = np.zeros(len(a), dtype=np.uint64)
    for j in range(m):
        f |= code[a + j] << np.uint64(2 * j)
        v |= (np.uint64(3) - code[a + m - 1 - j]) << np.uint64(2 * j)
    return f, v, (a + m - 1).astype(np.int64)


def ref_string_filter(concat, ends, m, log2, canonical):
    """FinDevIndex::cbf (canonical) / fbf: uint32 [2^log2, 4]"""
    f, v, _ = string_keys(concat, ends, m)
    key = np.minimum(f, v) if canonical else f
    h = key.copy()
    h ^= h >> np.uint64(29); h *= np.uint64(0xBF58476D1CE4E5B9); h ^= h >> np.uint64(32); h *= np.uint64(0x94D049BB133111EB); h ^= h >> np.uint64(29)
    block = ((h >> np.uint64(35)) & np.uint64((1 << log2) - 1)).astype(np.int64)
    words = np.zeros(4 << log2, dtype=np.uint32)
    for i in range(FIN_CBF_BITS):
        p = ((h >> np.uint64(7 * i)) & np.uint64(127)).astype(np.int64)
        np.bitwise_or.at(words, 4 * block + (p >> 5), (np.uint32(1) << (p & 31).astype(np.uint32)))
    return words.reshape(-1, 4)


def ref_absence_filter(concat, ends, F):
    """FinDevIndex::filt: 4^F bits as uint32 words, bit key set iff the string with that key lies inside one unitig"""
    f, _, _ = string_keys(concat, ends, F)
    words = np.zeros((1 << (2 * F)) // 32, dtype=np.uint32)
    np.bitwise_or.at(words, (f >> np.uint64(5)).astype(np.int64), np.uint32(1) << (f & np.uint64(31)).astype(np.uint32))
    return words


def ref_prefix_intervals(C, planes, n_nodes, T):
    """FinDevIndex::ptab / jtab: the SBWT search from [0, n_nodes - 1] for all 4^T keys at once, l <- C[c] + rank_c(l), r <- C[c] + rank_c(r + 1) - 1 with
    c = base i of the key (bits 2i); planes[c] = one 0/1 per node.  Returns (l, r, nonempty), int64 / bool [4^T]; l and r mean nothing where nonempty is false"""
    cum = np.zeros((4, n_nodes + 1), dtype=np.int64)
    for c in range(4):
        cum[c, 1:] = np.cumsum(np.asarray(planes[c][:n_nodes], dtype=np.int64))
    C = np.asarray(C, dtype=np.int64)
    keys = np.arange(1 << (2 * T), dtype=np.int64)
    l = np.zeros(len(keys), dtype=np.int64); r = np.full(len(keys), n_nodes - 1, dtype=np.int64)
    alive = np.ones(len(keys), dtype=bool)
    for i in range(T):
        c = (keys >> (2 * i)) & 3
        nl = C[c] + cum[c, l]; nr = C[c] + cum[c, r + 1] - 1
        alive &= nl <= nr
        l = np.where(alive, nl, 0); r = np.where(alive, nr, 0)
    return l, r, alive


def kmer_ends(ends, k):
    """the text positions that end a k-mer inside a unitig, ascending"""
    ends = np.asarray(ends, dtype=np.int64)
    starts = np.concatenate([[0], ends[:-1]])
    return np.concatenate([np.arange(s + k - 1, e) for s, e in zip(starts, ends)] + [np.zeros(0, np.int64)]).astype(np.int64)


def ref_safe(oracle, text, ends, k):
    """FinDevIndex::safe on the positions that end a k-mer: (those positions, uint8 bit per position) -- the bit is set iff the oracle's search of that k-mer alone
    reports the place that ends there"""
    ends = np.asarray(ends, dtype=np.int64)
    starts = np.concatenate([[0], ends[:-1]])
    at = kmer_ends(ends, k)
    answer = {}
    bit = np.zeros(len(at), dtype=np.uint8)
    for i, g in enumerate(at):
        q = text[g - k + 1:g + 1]
        if q not in answer:
            (u, off), = oracle.search(q)[0]
            answer[q] = int(starts[u]) + off + k - 1 if u >= 0 else -1
        bit[i] = answer[q] == g
    return at, bit


def ref_rcwin(text, ends, k):
    """FinDevIndex::rcwin: (uint8 [ceil(len / 512)], the number of k-mer places whose k-mer has its reverse complement among the k-mers of the text)"""
    at = kmer_ends(ends, k)
    kmers = {text[g - k + 1:g + 1] for g in at}
    win = np.zeros((len(text) + 511) // 512, dtype=np.uint8)
    n = 0
    for g in at:
        if rc(text[g - k + 1:g + 1]) in kmers:
            win[g >> 9] |= 1 << ((g >> 6) & 7)
            n += 1
    return win, n


def bits_at(words, at):
    """bits `at` of a bitmap given as uint64 words"""
    at = np.asarray(at, dtype=np.int64)
    return ((np.asarray(words, dtype=np.uint64)[at >> 6] >> (at & 63).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)


def bit_table_diff(got, want):
    """two bit tables of the same shape, two-sided: {'lacking': bits the definition sets and `got` does not -- a missing entry, a correctness bug --,
    'extra': bits `got` sets and the definition does not -- a precision bug --, 'first_lacking' / 'first_extra': the flat word index of the first such word or None}"""
    got = np.asarray(got).reshape(-1); want = np.asarray(want).reshape(-1)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    lack = want & ~got; extra = got & ~want
    cnt = lambda a: int(np.unpackbits(a.view(np.uint8)).sum())
    first = lambda a: int(np.nonzero(a)[0][0]) if a.any() else None
    return {"lacking": cnt(lack), "extra": cnt(extra), "first_lacking": first(lack), "first_extra": first(extra)}


def assert_bit_tables_equal(got, want, what):
    d = bit_table_diff(got, want)
    assert d["lacking"] == 0 and d["extra"] == 0, ("%s: the device lacks %d bits the definition sets (first in word %s): entries are MISSING, a correctness bug; "
                                                  "it sets %d bits the definition does not (first in word %s): a precision bug" %
                                                  (what, d["lacking"], d["first_lacking"], d["extra"], d["first_extra"]))


def interval_table_diff(tab, l, r, nonempty):
    """keys at which an interval table [4^T, 2] disagrees with ref_prefix_intervals: (l, r) equal where the definition's interval is non-empty, l > r elsewhere"""
    tab = np.asarray(tab, dtype=np.int64)
    bad = np.where(nonempty, (tab[:, 0] != l) | (tab[:, 1] != r), ~(tab[:, 0] > tab[:, 1]))
    return np.nonzero(bad)[0]


# ---- the unitig sets the upload-table tests run on (tests/test_upload_tables.py on the device, tests/test_upload_tables_host.py asserts the classes) --------------
# A builder lane takes 512 text positions, so what matters is where unitigs and strings lie against the multiples of 512 -- in the INDEX's order of the unitigs
# (by first k-mer, colexicographically; equal ones by input number).  Shortening a unitig at its end keeps its first k-mer, hence the order: that is how a set is
# made to measure.
UPLOAD_SEG = 512
UPLOAD_KS = (12, 16, 21, 31, 32, 33, 63, 100)


def _index_order(unitigs, k):
    return sorted(range(len(unitigs)), key=lambda i: (unitigs[i][:k][::-1], i))


def _shorten(unitigs, k, which, excess):
    """take `excess` bases off the ends of the unitigs `which`, in that order (none below k bases); False: they have not that many to give"""
    for i in which:
        cut = min(excess, len(unitigs[i]) - k)
        if cut:
            unitigs[i] = unitigs[i][:len(unitigs[i]) - cut]; excess -= cut
        if not excess:
            return True
    return False


def end_a_unitig_at(unitigs, k, at, spare=()):
    """a copy of the set in which, in the index's order, a unitig ends exactly at text position `at`: the unitigs in front of the one that crossed it are
    shortened (the nearest first, none of `spare`), then that one.  (the copy, that unitig's number), or None: impossible"""
    unitigs = list(unitigs)
    order = _index_order(unitigs, k); cum = 0
    for j, i in enumerate(order):
        cum += len(unitigs[i])
        if cum >= at:
            return (unitigs, i) if _shorten(unitigs, k, [x for x in reversed(order[:j]) if x not in spare] + [i], cum - at) else None
    return None


def fit_total(unitigs, k, total):
    unitigs = list(unitigs)
    assert _shorten(unitigs, k, list(reversed(_index_order(unitigs, k))), sum(len(u) for u in unitigs) - total), "the set cannot be cut down to %d bases" % total
    return unitigs


_UPLOAD_CASES = None


def upload_table_cases():
    """the unitig sets, made once: a list of namespaces (name, k, unitigs); nobody changes them.  Per k of UPLOAD_KS a "general" set -- a unitig of more than 1024
    bases, a dozen of k .. k + 8 bases, one of exactly k, pieces of a genome in either orientation, a unitig made to end on a multiple of 512 with at least 2k - 1
    bases, 2k + 10 bases in the first and the last unitig of the index's order --; sets whose whole text has k, 511, 512, 513 and a multiple of 512 plus m - 2 bases (m: the string filters' default length); sets of the deferral
    family (identical unitigs, near-duplicates, duplicated stretches, reverse-complement copies); disjoint sets with reverse-complement copies and, k even, a k-mer
    that is its own reverse complement; tiny sets at k = 4, 5 and 9 for interval tables as deep as k and k - 1"""
    global _UPLOAD_CASES
    if _UPLOAD_CASES is not None:
        return _UPLOAD_CASES
    from types import SimpleNamespace
    cases = []
    add = lambda name, k, unitigs: cases.append(SimpleNamespace(name=name, k=k, unitigs=tuple(unitigs)))
    for k in UPLOAD_KS:
        rng = np.random.default_rng(9000 + k)
        us = [random_genome(rng, 1300)] + [random_genome(rng, k + int(rng.integers(0, 9))) for _ in range(12)] + [random_genome(rng, k)]
        us += cut_unitigs(rng, random_genome(rng, 1500), k, max_len=3 * k + 100, flip=True)
        # the first and the last unitig of the index's order (their first k-mers end with AAAA / TTTT), with room for 2k - 1 bases and more
        us += [random_genome(rng, k - 4) + end * 4 + random_genome(rng, k + 14) for end in "AT"]
        done = None
        for at in range(UPLOAD_SEG, sum(len(u) for u in us), UPLOAD_SEG):   # the first multiple at which the unitig that ends there has 2k - 1 bases
            cut = end_a_unitig_at(us, k, at, spare=(0, len(us) - 2, len(us) - 1))
            if cut and len(cut[0][cut[1]]) >= 2 * k - 1 and cut[1] != 0:
                done = cut[0]
                break
        assert done is not None
        add("general_k%d" % k, k, done)
    for k, total in ((12, 12), (12, 511), (12, 512), (12, 513), (12, 2 * UPLOAD_SEG + default_cbf_m(12) - 2), (31, UPLOAD_SEG + default_cbf_m(31) - 2),
                     (63, 2 * UPLOAD_SEG + default_cbf_m(63) - 2)):
        rng = np.random.default_rng(9500 + 7 * k + total)
        us = [random_genome(rng, k)] if total == k else fit_total(cut_unitigs(rng, random_genome(rng, total + 10), k, max_len=max(90, 4 * k), flip=True), k, total)
        add("total_%d_k%d" % (total, k), k, us)
    for k, case in ((12, 3), (21, 4), (33, 1), (63, 2)):
        rng = np.random.default_rng(9700 + k)
        add("family_k%d" % k, k, defer_family_case(rng, case, k, n_reads=3)[1])
    for k in (12, 16, 21, 32):
        rng = np.random.default_rng(9800 + k)
        g = random_genome(rng, 1200)
        us = cut_unitigs(rng, g, k, max_len=4 * k + 60, flip=False) + [rc(g[200:200 + 5 * k])]   # (one orientation: the copy's k-mers are in no other unitig)
        if k % 2 == 0:
            w = random_genome(rng, k // 2)
            us.append(random_genome(rng, 7) + w + rc(w) + random_genome(rng, 7))
        add("rc_k%d" % k, k, us)
    for k in (4, 5, 9):
        rng = np.random.default_rng(9900 + k)
        add("tiny_k%d" % k, k, cut_unitigs(rng, random_genome(rng, 300), k, max_len=40, flip=True))
    _UPLOAD_CASES = cases
    return cases


def upload_case(name):
    return next(c for c in upload_table_cases() if c.name == name)


_UPLOAD_HOST = {}


def upload_case_host(case):
    """what the references need of a case, from the host builder and the oracle, made once per case and shared: concat (codes), text, ends, starts, C, planes
    (0/1 per node), n_nodes, oracle.  The oracle's own index of the same unitigs must be the exported one"""
    if case.name not in _UPLOAD_HOST:
        from types import SimpleNamespace
        import finito_amd as fa
        from oracle.oracle import OracleIndex
        p = fa.FinimizerIndex.build(list(case.unitigs), case.k)
        concat = p.export(fa.X_CONCAT); ends = p.export(fa.X_ENDS).astype(np.int64); n = p.n_nodes
        planes = [unpack_bits(p.export(fa.X_PLANE_A + c), n) for c in range(4)]
        C = p.export(fa.X_C)[:4].astype(np.int64)
        p.close()
        o = OracleIndex.build(list(case.unitigs), case.k)
        assert np.array_equal(o.concat(), concat) and np.array_equal(o.ends(), ends)
        for a in (concat, ends, C):
            a.setflags(write=False)
        _UPLOAD_HOST[case.name] = SimpleNamespace(concat=concat, text=text_of(concat), ends=ends, starts=np.concatenate([[0], ends[:-1]]), C=C, planes=planes, n_nodes=n,
                                                  oracle=o, memo={})
    return _UPLOAD_HOST[case.name]


def yes_reads(text, k, a, b):
    """reads that follow unitig A = text[a[0]:a[1]] for k + 5 bases (its last ones, or first ones) and carry 2k - 1 bases of B = text[b[0]:b[1]] at every offset:
    both orders, both strands"""
    A = text[a[0]:a[1]]; B = text[b[0]:b[1]]
    n = min(len(A), k + 5)
    reads = []
    for o in range(len(B) - (2 * k - 1) + 1):
        piece = B[o:o + 2 * k - 1]
        for r in (A[-n:] + piece, piece + A[:n]):
            reads += [r, rc(r)]
    return reads


# ---- the enumerated digit case (tests/test_record_digits_host.py asserts its conditions, tests/test_record_digits.py gives it to the device) ----------------------
# fin_batch_set_records checks neither u nor off0, and text, segments, read summaries and the record gather have no notion of the index: records may name any unitig
# number up to 2^31 - 1 at any offset.  The kind-1 records here are ENUMERATED -- every digit count of the unitig number against every boundary of the offset at
# which fin_text.hip's arithmetic changes (a digit more, another H = offset / 1000, H + 1 longer than H), at every nk that puts the boundary into the first group of
# 128 pairs, at slot 127 / 128 and into the third group -- and thinned by strides, not by drawing; only the searched reads' pairs and the filler positions are drawn.
DIGIT_K = 31
INT32_MAX = 2 ** 31 - 1
DIGIT_NKS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 270)
DIGIT_NES = (0, 1, 4, 5, 8)
DIGIT_H_GAINS = (9, 99, 999, 9999, 99999, 999999)      # H + 1 has a digit more than H
DIGIT_BOUNDARIES = tuple(sorted({10 ** e for e in range(1, 10)} | {2 ** 31, 1000, 2000, 123000, 7654000} | {1000 * (H + 1) for H in DIGIT_H_GAINS}))
DIGIT_LOW_ENDS = (9, 10, 99, 100, 999)                 # last offsets of reads below 1000: one to three digits and no H
DIGIT_SHAPES = (7, 8, 3, 4, 1, 7, 8, 5, 0, 6, 2)       # _record_positions' shapes, in the order the enumeration hands them out
DIGIT_RUN = (512, 768)                                  # the reads of the run on one 6-digit unitig
DIGIT_RUN_UNITIG = 314159
DIGIT_LONG = ((4097, 0, 10 ** 6 - 2000), (9001, 0, 10 ** 9 - 5000), (4097, 1, 10 ** 9 - 4000), (9001, 1, 10 ** 6 - 8000))   # (nk, strand, off0)
DIGIT_LONG_UNITIG = 1987654321
DIGIT_MAX_READS = 16                                    # per kind: reads of 24-byte pairs only, one made to start at each byte offset modulo 16
_WAVE_KIND0, _WAVE_KIND2 = (5, 21, 37, 53), (11, 43)    # places inside every wave of 64 reads
_WAVE_MAX, _WAVE_LONG = (30, 60), 50                    # a 24-byte read (its filler one place in front of it); a long read


def digit_unitig_numbers():
    """per digit count 1..10: the smallest number, one in between, the largest (2^31 - 1 caps the ten-digit ones)"""
    out = []
    for n in range(1, 11):
        lo, hi = (0 if n == 1 else 10 ** (n - 1)), min(10 ** n - 1, INT32_MAX)
        out += [lo, lo + (hi - lo) * 3 // 7, hi]
    return out


def digit_offsets(nk):
    """[(off0, P)]: off0 = 0, the reads that end on DIGIT_LOW_ENDS (P None), and the five places against every boundary P; what would leave int32 is left out"""
    out = [(0, None)] + [(e - nk + 1, None) for e in DIGIT_LOW_ENDS]
    for P in DIGIT_BOUNDARIES:
        out += [(o, P) for o in (P - nk, P - nk + 1, P - nk // 2, P - 1, P)]
    seen, kept = set(), []
    for o, P in out:
        if o >= 0 and o + nk - 1 <= INT32_MAX and (o, P) not in seen:
            seen.add((o, P)); kept.append((o, P))
    return kept


def _positions_at(rng, nk, k, nE, shape, s):
    """_record_positions and two shapes "around slot s" (s = None: shape 0 instead): 7 a gap that covers slot s, the others anywhere within 2k of it; 8 a gap that
    ends just before slot s, which stays found (the others lie in front of it)"""
    top = nk + k - 2
    if nE == 0 or shape < 7:
        return _record_positions(rng, nk, k, nE, shape)
    if s is None or (shape == 8 and s == 0):
        return _record_positions(rng, nk, k, nE, 0)
    if shape == 7:
        E = [s + int(rng.integers(0, k))] + [int(x) for x in rng.integers(max(0, s - 2 * k), s + 2 * k + 1, nE - 1)]
    else:
        E = [s - 1] + [int(x) for x in rng.integers(0, s, nE - 1)]
    return sorted(min(x, top) for x in E)


def _set_record(rec, u, off0, nk, rev, Es):
    rec["u"], rec["off0"], rec["nk"], rec["meta"] = u, off0, nk, len(Es) | (rev << 8) | (1 << 16)
    rec["Es"] = sum(E << (16 * e) for e, E in enumerate(Es[:4])); rec["Es2"] = sum(E << (16 * e) for e, E in enumerate(Es[4:]))


def arbitrary_pairs(rng, n, absent):
    """the generator of tests/test_search_gpu.py::test_output_text_of_arbitrary_pairs: numbers of 1..10 digits in both fields, a share `absent` of (-1,-1)"""
    digits = rng.integers(1, 11, (n, 2))
    vals = np.minimum((10.0 ** (digits - rng.random((n, 2)))).astype(np.int64), INT32_MAX).astype(np.int32)
    vals[rng.random(n) < absent] = -1
    return vals


def pair_text_len(pairs):
    """bytes of every pair's text, separator included: int64 [n]"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    nd = lambda v: np.searchsorted(10 ** np.arange(1, 10), np.maximum(v, 0), side="right") + 1
    return np.where(p[:, 0] < 0, 8, nd(p[:, 0]) + nd(p[:, 1]) + 4)


_DIGIT_CASE = None


def digit_case():
    """the one input tests/test_record_digits_host.py (no GPU) and tests/test_record_digits.py face: a 40 000-base genome's index at k = 31, reads whose content is
    free (they fix nk), and over them
      - the enumerated kind-1 records: (boundary, place against it, nk, strand) in full, the unitig number and (number of positions, shape) handed out by strides;
      - reads DIGIT_RUN: kind 1 on ONE 6-digit unitig; four long reads (DIGIT_LONG) on a 10-digit unitig across 10^6 and 10^9;
      - 2 * DIGIT_MAX_READS reads whose pairs all take 24 bytes -- searched ones of 260 pairs (2147483647,2147483647), finished ones of 257 slots that end on
        offset 2^31 - 1 of unitig 2^31 - 1 --, each behind a one-pair filler read chosen so that the j-th of its kind starts at byte j modulo 16 of the text;
      - in every wave of 64 reads outside the run four searched reads of arbitrary_pairs and two kind-2 reads.
    Namespace: k, unitigs, ends, reads, nks, recs, stream, pairs (brute_expand), boundary (per read: its P or -1).  Made once and shared; nobody changes it"""
    global _DIGIT_CASE
    if _DIGIT_CASE is not None:
        return _DIGIT_CASE
    from types import SimpleNamespace
    import finito_amd as fa
    from oracle.oracle import OracleIndex
    from tests.test_records import brute_expand
    k = DIGIT_K
    rng = np.random.default_rng(7031)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=700)
    ends = OracleIndex.build(unitigs, k).ends()
    numbers = digit_unitig_numbers()
    # the enumeration: boundary and place, nk, strand in full; one unitig number per (place, nk), the same on both strands, by a stride coprime to their count
    specs = []
    for nk in DIGIT_NKS:
        for off0, P in digit_offsets(nk):
            for rev in (0, 1):
                specs.append((off0, P, nk, rev))
    specs.sort(key=lambda x: (x[1] is not None, x[1] or 0, x[0], x[2], x[3]))
    one = []
    for i, (off0, P, nk, rev) in enumerate(specs):
        u = numbers[(11 * (i // 2)) % len(numbers)]
        nE, shape = DIGIT_NES[i % 5], DIGIT_SHAPES[(i // 5) % len(DIGIT_SHAPES)]
        s = None
        if P is not None:   # the slot at P - 1 or at P, alternately, whichever the read has
            s = [x for x in ((P - 1 - off0, P - off0) if (i // 55) % 2 == 0 else (P - off0, P - 1 - off0)) if 0 <= x < nk]
            s = s[0] if s else None
        one.append((u, off0, nk, rev, _positions_at(rng, nk, k, nE, shape, s), -1 if P is None else P))
    # the layout: kinds 0 and 2 at fixed places of every wave, the run, the 24-byte reads behind their fillers, the long reads; kind 1 everywhere else
    n_special = 2 * 2 * DIGIT_MAX_READS + len(DIGIT_LONG)
    per_wave = 64 - len(_WAVE_KIND0) - len(_WAVE_KIND2)
    n_waves = (len(one) + n_special + per_wave - 1) // per_wave + (DIGIT_RUN[1] - DIGIT_RUN[0]) // 64
    n = 64 * n_waves
    run_waves = set(range(DIGIT_RUN[0] // 64, DIGIT_RUN[1] // 64))
    free = [w for w in range(n_waves) if w not in run_waves]
    assert len(free) >= DIGIT_MAX_READS + len(DIGIT_LONG)
    plan = {}
    for j in range(2 * DIGIT_MAX_READS):   # two per wave: a searched one, a finished one
        at = 64 * free[j // 2] + _WAVE_MAX[j % 2]
        plan[at - 1], plan[at] = ("filler", j), ("max0" if j % 2 == 0 else "max1", j // 2)
    for j, spec in enumerate(DIGIT_LONG):
        plan[64 * free[len(free) - 1 - j] + _WAVE_LONG] = ("long", spec)
    recs = np.zeros(n, dtype=fa.RECORD_DTYPE)
    boundary = np.full(n, -1, dtype=np.int64)
    stream_of, fillers, maxes = {}, [], []
    next_one = next_nk = 0
    for r in range(n):
        w, at = divmod(r, 64)
        if DIGIT_RUN[0] <= r < DIGIT_RUN[1]:
            j = r - DIGIT_RUN[0]
            nk = DIGIT_NKS[j % len(DIGIT_NKS)]
            off0 = (999, 9999, 99999, 123456, 999999)[j % 5] - (j % 7) * (nk // 6)
            _set_record(recs[r:r + 1], DIGIT_RUN_UNITIG, max(off0, 0), nk, (j // 3) % 2, _record_positions(rng, nk, k, DIGIT_NES[j % 5], j % POSITION_SHAPES))
        elif r in plan:
            what, arg = plan[r]
            if what == "filler":
                recs["nk"][r] = 1; stream_of[r] = np.array([[1, 1]], dtype=np.int32); fillers.append(r)
            elif what == "max0":
                recs["nk"][r] = 260 + arg % 11; stream_of[r] = np.full((260 + arg % 11, 2), INT32_MAX, dtype=np.int32); maxes.append(r)
            elif what == "max1":
                _set_record(recs[r:r + 1], INT32_MAX, 2 ** 31 - 257, 257, arg % 2, []); maxes.append(r)
            else:
                nk, rev, off0 = arg
                P = 10 ** 6 if off0 < 10 ** 6 else 10 ** 9
                _set_record(recs[r:r + 1], DIGIT_LONG_UNITIG, off0, nk, rev, _positions_at(rng, nk, k, (0, 8, 5, 4)[DIGIT_LONG.index(arg)], 7, P - off0))
        elif at in _WAVE_KIND0:
            nk = DIGIT_NKS[next_nk % len(DIGIT_NKS)]; next_nk += 1
            recs["nk"][r] = nk; stream_of[r] = arbitrary_pairs(rng, nk, (0.0, 0.3, 0.9)[next_nk % 3])
        elif at in _WAVE_KIND2:
            recs["nk"][r] = DIGIT_NKS[next_nk % len(DIGIT_NKS)]; next_nk += 1
            recs["meta"][r] = 2 << 16
        else:
            u, off0, nk, rev, Es, P = one[next_one % len(one)]; next_one += 1   # (the last wave is filled up from the start of the enumeration)
            _set_record(recs[r:r + 1], u, off0, nk, rev, Es); boundary[r] = P
    assert next_one >= len(one), "the enumeration did not fit: %d of %d" % (next_one, len(one))
    # the fillers, in read order: a pair of 6 .. 21 bytes that puts the read behind it at its byte offset modulo 16
    nks = recs["nk"].astype(np.int64)
    zero = [r for r in range(n) if int(recs["meta"][r]) >> 16 == 0]
    stream = np.concatenate([stream_of[r] for r in zero]).astype(np.int32)
    in_stream = dict(zip(zero, np.concatenate([[0], np.cumsum(nks[zero])])))
    pairs = brute_expand(recs, stream, k)
    first = np.concatenate([[0], np.cumsum(nks)])
    length = np.add.reduceat(pair_text_len(pairs), first[:-1])
    for f, m in zip(fillers, maxes):
        assert m == f + 1
        want = plan[m][1] % 16
        fill = 6 + (want - int(length[:f].sum()) - 6) % 16
        nu = min(10, fill - 5)
        stream[in_stream[f]] = pairs[first[f]] = (10 ** (nu - 1), 10 ** (fill - 4 - nu - 1))
        length[f] = fill
    assert np.array_equal(np.add.reduceat(pair_text_len(pairs), first[:-1]), length)
    for m in maxes:
        assert int(length[:m].sum()) % 16 == plan[m][1] % 16
    lens = nks + k - 1
    bases = rng.integers(0, 4, int(lens.sum()))
    reads, at = [], 0
    for L in lens:
        reads.append("".join("ACGT"[x] for x in bases[at:at + L])); at += int(L)
    for a in (ends, nks, recs, stream, pairs, boundary):
        a.setflags(write=False)
    _DIGIT_CASE = SimpleNamespace(k=k, unitigs=unitigs, ends=ends, reads=reads, nks=nks, recs=recs, stream=stream, pairs=pairs, boundary=boundary)
    return _DIGIT_CASE


# ---- constructed colliders of the compact k-mer table (finito_amd/csrc/fin_format.h: FinDevIndex::kt3, fin_kt3_hash) --------------------------------------------
# The table holds no k-mer: a slot is {answer g, 30-bit tag}, the bucket comes from the hash's high word, and a tag match is a claim that only the text at g proves.
# fin_mix64 is a bijection and fin_kt3_hash(k0, k1 ...) = fin_mix64(k0 ^ fold(k1 ...)): for a k-mer y, h' = h(y) ^ (d << 30), d = 1, 2, 3, keeps the high word (the
# bucket, for ANY number of buckets) and the low 30 bits (the tag), and k0' = mix64^-1(h') ^ fold(k1 ...) is the first key word of a k-mer x != y with that hash.
# Any 64-bit k0' is a k-mer's first word for k >= 32; for k = 31 it must lie below 2^62.  (No control over how far x lies from y: a collider a base or two from
# its victim -- a sibling -- cannot be made this way.)  tests/test_kmer_table_collisions_host.py holds these restatements against the header itself.
KT3_FOLD = 0x9E3779B97F4A7C15
KT3_TAG_BITS = 30
_MIX_A, _MIX_B = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_MIX_A_INV, _MIX_B_INV = pow(_MIX_A, -1, 1 << 64), pow(_MIX_B, -1, 1 << 64)


def mix64(x):
    """fin_mix64 on a Python integer"""
    x ^= x >> 29; x = (x * _MIX_A) & _M64; x ^= x >> 32; x = (x * _MIX_B) & _M64; x ^= x >> 29
    return x


def unmix64(h):
    """the inverse of fin_mix64: every step undone in reverse order (x ^= x >> 29 is undone by x ^= x >> 29 ^ x >> 58, x ^= x >> 32 by itself)"""
    h ^= (h >> 29) ^ (h >> 58); h = (h * _MIX_B_INV) & _M64; h ^= h >> 32; h = (h * _MIX_A_INV) & _M64; h ^= (h >> 29) ^ (h >> 58)
    return h


def kmer_words(s):
    """the key words of a k-mer: word j = bases 32 j .. 32 j + 31, the first base in the low bits (2-bit codes A0 C1 G2 T3)"""
    return [string_key(s[a:a + 32]) for a in range(0, len(s), 32)]


def words_kmer(words, k):
    return "".join("ACGT"[(words[j >> 5] >> (2 * (j & 31))) & 3] for j in range(k))


def kt3_fold(key, word, j):
    """fin_kt3_fold: word j >= 1 enters the key as a finaliser of itself plus j times the constant; a word of zeros adds nothing"""
    return key ^ mix64((word + KT3_FOLD * j) & _M64) if word else key


def kt3_key(words):
    key = words[0]
    for j in range(1, len(words)):
        key = kt3_fold(key, words[j], j)
    return key


def kt3_hash(words):
    """fin_kt3_hash of a k-mer given as its key words (any number of them; one or two: the two-word form of the header)"""
    return mix64(kt3_key(words))


def kt3_bucket(h, n_buckets):
    """fin_kt3_bucket"""
    return ((h >> 32) * n_buckets) >> 32


def _with_hash(kmer, h):
    """the k-mer that keeps every key word of `kmer` but the first and hashes to h; None: that first word is no k-mer's (k < 32)"""
    words = kmer_words(kmer)
    w0 = unmix64(h) ^ kt3_key(words) ^ words[0]
    if len(kmer) < 32 and w0 >> (2 * len(kmer)):
        return None
    return words_kmer([w0] + words[1:], len(kmer))


def colliders_of(kmer):
    """the valid k-mers (up to three) whose hash differs from this k-mer's in bits 30 and 31 only: the same bucket in a table of any size, the same tag"""
    h = kt3_hash(kmer_words(kmer))
    return [x for x in (_with_hash(kmer, h ^ (d << KT3_TAG_BITS)) for d in (1, 2, 3)) if x is not None]


def control_of(kmer):
    """a valid k-mer with this k-mer's high hash word -- its bucket -- and ANOTHER tag: the lowest tag bit flipped; k = 31, where three first words in four are no
    k-mer's (not below 2^62): the first of the masks 1, 2, 3 ... over the low tag bits that gives one"""
    h = kt3_hash(kmer_words(kmer))
    for mask in range(1, 1 << 12):
        x = _with_hash(kmer, h ^ mask)
        if x is not None:
            return x
    raise AssertionError("no control for %s" % kmer)


# The cases of tests/test_kmer_table_collisions.py (device) and tests/test_kmer_table_collisions_host.py (what each presupposes, asserted on the CPU).  A read is
# a list of parts -- strings, and ("K", k-mer) for a member of a tag group --, reverse-complemented or not: the CONTROL batch is the same reads with every such
# member replaced by control_of (same bucket, another tag).  A look-up of the walk kernel comes behind probes that passed: a k-mer none of whose strings is in a unitig
# is settled by the string filters and never reaches the table (measured with bare colliders: kernel 3's list stayed empty in scenario 1 at k = 31, 32 and 100 and
# in scenario 2 at k = 31, 32, 64 and 100).  So every absent collider AND every control k-mer has all its strings of k - 1 bases in the index (_support; scenario 4:
# the whole run, with the collider and with its control): both get past the probes to the same bucket, and what the two batches send to kernel 3 differs by the
# tag alone.  collision_case_problems asserts on the CPU that these strings are in the filters and that the k-mers are absent.
COLLISION_KS = (31, 32, 63, 64, 100, 127, 200)
COLLISION_SCENARIOS = {1: "absent collider, verified victim", 2: "where the claimed place lies", 3: "present collider", 4: "runs of absent k-mers whose strings all occur",
                       5: "unverified victim"}
_COLLISION_CASES = {}


def collision_scenarios(k):
    return (1, 2, 3) if k == 200 else (1, 2, 3, 4, 5) if k == 31 else (1, 2, 3, 5)


def prepass_middle_start(read_len, k):
    """where the k-mer starts that the fast pre-pass looks at third (fin_prepass.hip, middle_look: the k-mer that ENDS at t = (r_len + k) / 2 - 1)"""
    return (read_len + k) // 2 - k


def render_read(spec, sub=None):
    parts, rev = spec
    s = "".join(p if isinstance(p, str) else (sub or {}).get(p[1], p[1]) for p in parts)
    return rc(s) if rev else s


def _placements(rng, g, k, x):
    """the reads that carry the k-mer x where a look or a look-up meets it: as the first, the last and the pre-pass's middle k-mer (junk around it: that look is made
    only when the first and the last k-mer of both strands are in no unitig), spliced between two stretches of the genome, alone, and twice; each on both strands.
    [(kind, spec)]"""
    def S():
        n = k + int(rng.integers(3, 40 if k < 40 else 25)); a = int(rng.integers(0, len(g) - n + 1))   # (k <= 64: no read beyond the fast path's 256 bases)
        return g[a:a + n]
    m = int(rng.integers(6, 30)); odd = int(rng.integers(0, 2))
    mid = [random_genome(rng, m), ("K", x), random_genome(rng, m + odd)]
    assert prepass_middle_start(2 * m + odd + k, k) == m
    out = [("first", [("K", x), S()]), ("last", [S(), ("K", x)]), ("middle", mid), ("spliced", [S(), ("K", x), S()]), ("whole", [("K", x)]), ("twice", [("K", x), S(), ("K", x)])]
    return [(kind, (parts, rev)) for kind, parts in out for rev in (False, True)]


def _along(rng, k, m, left, right):
    """reads along the text around a k-mer m that IS in the index (left / right: the bases on its sides there): the whole stretch, from m on, up to m, m alone"""
    out = [("along", [left, ("K", m), right]), ("first", [("K", m), right]), ("last", [left, ("K", m)]), ("whole", [("K", m)])]
    return [(kind, (parts, rev)) for kind, parts in out for rev in (False, True)]


def _support(rng, k, s):
    """unitigs of k bases that hold every string of k - 1 bases of s and none of its k-mers: each string goes on with another base than s does -- with C or G, so that
    in the index's order (by first k-mer, from its last base) none of them becomes the first or the last unitig of the text (scenario 2 needs those for its victims)"""
    out = []
    for i in range(len(s) - k + 2):
        nxt = s[i + k - 1] if i + k - 1 < len(s) else ""
        ok = [b for b in "CG" if b != nxt]
        out.append(s[i:i + k - 1] + ok[int(rng.integers(0, len(ok)))])
    return out


def _answers(o, text, ends, k, kmers):
    """per k-mer: (the text position g the oracle's search of the k-mer alone answers, or -1; does the text spell the k-mer there, inside one unitig)"""
    starts = np.concatenate([[0], ends[:-1]])
    out = {}
    for q in kmers:
        (u, off), = o.search(q)[0]
        g = int(starts[u]) + off + k - 1 if u >= 0 else -1
        out[q] = (g, u >= 0 and off + k <= int(ends[u] - starts[u]) and text[g - k + 1:g + 1] == q)
    return out


def _collision_try(k, scenario, seed):
    from types import SimpleNamespace
    from oracle.oracle import OracleIndex
    rng = np.random.default_rng(seed)
    g = random_genome(rng, int(rng.integers(3000, 6001)))
    if scenario == 5:   # duplicated stretches: answers that do not spell their k-mer (tests/test_search_gpu.py::test_compact_kmer_table_k_mer_by_k_mer, cases 2-4)
        for _ in range(6):
            a = int(rng.integers(0, len(g) - 300 - k)); n = int(rng.integers(k + 3, k + 300)); at = int(rng.integers(0, len(g)))
            g = g[:at] + g[a:a + n] + g[at:]
    base = cut_unitigs(rng, g, k, max_len=max(200, 2 * k + 100))
    o = OracleIndex.build(base, k)
    ends = np.asarray(o.ends(), dtype=np.int64); starts = np.concatenate([[0], ends[:-1]]); text = text_of(o.concat())
    at = kmer_ends(ends, k)
    n_col = 3 if k >= 32 else 1
    has = lambda q: len(colliders_of(q)) >= 1
    where = {}
    # ---- the victims (k-mers of the text), by scenario
    if scenario == 2:
        u = next((u for u in range(1, len(ends) - 1) if has(text[starts[u]:starts[u] + k]) and has(text[ends[u] - k:ends[u]]) and ends[u] - starts[u] > k), None)
        if u is None:
            return None
        where = {"text_first": k - 1, "text_last": len(text) - 1, "unitig_first": int(starts[u]) + k - 1, "unitig_last": int(ends[u]) - 1}
        if k == 31:   # the claimed place inside one 64-base text window (the walk kernel compares in W_RES4), and across two (W_KFV)
            one = [int(e) for e in at if ((e - k + 1) & 63) + k <= 64 and has(text[e - k + 1:e + 1]) and e not in where.values()]
            two = [int(e) for e in at if ((e - k + 1) & 63) + k > 64 and has(text[e - k + 1:e + 1]) and e not in where.values()]
            if not one or not two:
                return None
            where["one_window"] = one[int(rng.integers(0, len(one)))]; where["two_windows"] = two[int(rng.integers(0, len(two)))]
        victims = [text[e - k + 1:e + 1] for e in where.values()]
    else:
        pool = [text[e - k + 1:e + 1] for e in at[rng.permutation(len(at))]]
        if scenario == 5:
            ans = _answers(o, text, ends, k, pool)
            pool = [q for q in pool if not ans[q][1]]
        pool = [q for q in dict.fromkeys(pool) if has(q)]
        want = {1: 8 if k >= 32 else 20, 3: 3, 4: 8, 5: 6}[scenario]
        victims = pool[:want]
        if len(victims) < want:
            return None
    if not all(has(v) for v in victims) or len(set(victims)) < len(victims):
        return None
    groups = [(v, colliders_of(v)[:n_col]) for v in victims]
    # ---- which colliders go into the index, the unitigs that carry them, and the reads
    extra, present, flanks, runs, reads = [], set(), {}, [], []
    add = lambda what, specs: reads.extend((what, kind, spec) for kind, spec in specs)
    if scenario in (1, 2):
        for v, cs in groups:
            for x in cs:
                add("absent", _placements(rng, g, k, x))
    elif scenario == 3:   # one collider present; (k >= 32) all three present: four entries of one tag in one chain
        for i, (v, cs) in enumerate(groups):
            groups[i] = (v, cs if i == 1 else cs[:1])
            present.update(groups[i][1])
    elif scenario == 5:   # half the victims meet an absent collider (a miss in the exact side table), half a present one
        for i, (v, cs) in enumerate(groups):
            groups[i] = (v, cs[:1])
            if i % 2:
                present.add(cs[0])
            else:
                add("absent", _placements(rng, g, k, cs[0]))
    if scenario == 4:   # R = J1 + x + J2: no k-mer of R is in the index, and every string of k - 1 bases of R is (_support, below)
        for v, cs in groups:
            x = cs[0]
            R = random_genome(rng, 3) + x + random_genome(rng, 12)   # (one run per collider; the reads enter it 0 .. 3 bases in front of x)
            runs.append(R)
            for n1 in range(4):
                parts = [R[3 - n1:3], ("K", x), R[3 + k:]]
                n = k + int(rng.integers(3, 40)); a = int(rng.integers(0, len(g) - n + 1)); b = int(rng.integers(0, len(g) - n + 1))
                # the run first in the read (x is the epoch's first look-up at n1 = 0, a later one behind n1 absent k-mers), and behind a stretch of the genome
                add("run", [("run_first", (parts + [g[a:a + n]], rev)) for rev in (False, True)] + [("run_inside", ([g[b:b + n]] + parts + [g[a:a + n]], rev)) for rev in (False, True)])
    for x in sorted(present):
        n = int(rng.integers(30, 80)) if k < 100 else int(rng.integers(10, 40))
        flanks[x] = (random_genome(rng, n), random_genome(rng, n))
        extra.append(flanks[x][0] + x + flanks[x][1])
    if present:
        for v, cs in groups:
            if any(x in present for x in cs):
                n = 40 if k < 100 else 25
                a = g.find(v)
                if a >= 0:
                    left, right = g[max(0, a - n):a], g[a + k:a + k + n]
                else:   # (the victim's unitig went into the set reverse-complemented)
                    a = g.find(rc(v))
                    left, right = rc(g[a + k:a + k + n]), rc(g[max(0, a - n):a])
                add("member", _along(rng, k, v, left, right))
                for x in cs:
                    if x in present:
                        add("member", _along(rng, k, x, *flanks[x]))
    members = list(dict.fromkeys(p[1] for _, _, spec in reads for p in spec[0] if not isinstance(p, str)))
    control = {m: control_of(m) for m in members}
    # what must get past the probes without being in the index: the absent colliders and the control k-mers (scenario 4: the runs, with either)
    victims_set = {v for v, _ in groups}
    supported = [m for m in members if m not in present and m not in victims_set] + list(control.values())
    if scenario == 4:
        supported = runs + [R.replace(cs[0], control[cs[0]]) for R, (v, cs) in zip(runs, groups)]
    for s_ in supported:
        extra += _support(rng, k, s_)
    unitigs = base + extra
    if extra:
        order = rng.permutation(len(unitigs)); unitigs = [unitigs[i] for i in order]
        o = OracleIndex.build(unitigs, k)
        ends = np.asarray(o.ends(), dtype=np.int64); text = text_of(o.concat())
        where = {name: text.find(v) + k - 1 for name, (v, _) in zip(where, groups)}   # (the new unitigs have their places in the index's order: the victims have moved)
    c = SimpleNamespace(k=k, scenario=scenario, seed=seed, genome=g, unitigs=tuple(unitigs), oracle=o, text=text, ends=ends, groups=groups, present=present, where=where,
                        flanks=flanks, runs=runs, supported=supported, control=control, kinds=[(what, kind, spec[1]) for what, kind, spec in reads], reads=[render_read(spec) for _, _, spec in reads],
                        control_reads=[render_read(spec, control) for _, _, spec in reads])
    c.answers = _answers(o, text, ends, k, [v for v, _ in groups] + [x for _, cs in groups for x in cs] + list(control.values()))
    if collision_case_problems(c):
        return None
    c.first_reads = [i for i, (what, kind, rev) in enumerate(c.kinds) if what == "absent" and kind == "first" and not rev]
    c.expected = {}
    for name, rd in (("reads", c.reads), ("control", c.control_reads)):
        merged = o.search_batch(rd)[0]
        fwd = np.array([x for r in rd for x in o.search(r)[0]], dtype=np.int64).reshape(-1, 2)
        merged.setflags(write=False); fwd.setflags(write=False)
        c.expected[name] = (merged, fwd)
    return c


def collision_case_problems(c):
    """what a case presupposes, on the CPU: every victim is in the text and answered as its scenario says (verified at its own place; scenario 5: at a place that does
    not spell it), a present collider is found at its own place, an absent collider and every control k-mer is found on neither strand; and of
    everything that must get past the probes -- absent colliders, control k-mers, scenario 4's runs with either -- no k-mer is in the index and every string of the
    filters' length is in a unitig.  Returns the list of what does not hold"""
    k, bad = c.k, []
    for v, cs in c.groups:
        g, spelled = c.answers[v]
        if g < 0 or spelled != (c.scenario != 5):
            bad.append(("victim", v, g, spelled))
        for x in cs:
            h, hv = kt3_hash(kmer_words(x)), kt3_hash(kmer_words(v))
            if x == v or (h ^ hv) & ~(3 << KT3_TAG_BITS):
                bad.append(("not a collider", v, x))
            gx, sx = c.answers[x]
            if x in c.present and not (gx >= 0 and sx):
                bad.append(("present collider", x, gx, sx))
            if x not in c.present and (gx >= 0 or c.oracle.search(rc(x))[0][0][0] >= 0):
                bad.append(("absent collider", x, gx))
    for m, q in c.control.items():
        hm, hq = kt3_hash(kmer_words(m)), kt3_hash(kmer_words(q))
        if hm >> 32 != hq >> 32 or not (hm ^ hq) & ((1 << KT3_TAG_BITS) - 1) or c.answers[q][0] >= 0 or c.oracle.search(rc(q))[0][0][0] >= 0:
            bad.append(("control", m, q))
    for name, e in c.where.items():
        v = c.groups[list(c.where).index(name)][0]
        if c.answers[v][0] != e or c.text[e - k + 1:e + 1] != v:
            bad.append(("place", name, e))
    if c.scenario == 2:
        w, starts = c.where, [0] + [int(e) for e in c.ends[:-1]]
        if w["text_first"] != k - 1 or w["text_last"] != len(c.text) - 1 or w["unitig_first"] - k + 1 not in starts[1:] or w["unitig_last"] + 1 not in [int(e) for e in c.ends[:-1]]:
            bad.append(("scenario 2's places", dict(w)))
        if k == 31 and not ((w["one_window"] - k + 1) & 63) + k <= 64 < ((w["two_windows"] - k + 1) & 63) + k:
            bad.append(("scenario 2's windows", dict(w)))
    m = default_cbf_m(k)
    strings = {c.text[e - m + 1:e + 1] for e in string_keys(c.oracle.concat(), c.ends, m)[2]}
    absent = [x for _, cs in c.groups for x in cs if x not in c.present] + list(c.control.values())
    if not set(absent) <= {R[i:i + k] for R in c.supported for i in range(len(R) - k + 1)}:
        bad.append(("an absent collider or a control k-mer without its strings in the index",))
    for R in c.supported:
        if any(R[i:i + m] not in strings for i in range(len(R) - m + 1)):
            bad.append(("a string is in no unitig", R))
        if any(u >= 0 for u, _ in c.oracle.search_merged(R)):
            bad.append(("a k-mer is in the index", R))
    return bad


def collision_case(k, scenario):
    """the one case of (k, scenario), made once and shared; nobody changes it.  Deterministic: the first seed of a fixed sequence whose draw has what the scenario
    presupposes (at k = 31 only some 55 % of the k-mers have a collider at all; a collider's unitig may disturb a neighbour's answer)"""
    if (k, scenario) not in _COLLISION_CASES:
        assert scenario in collision_scenarios(k)
        for t in range(60):
            c = _collision_try(k, scenario, 31000 + 1000 * scenario + 10 * k + 100000 * t)
            if c is not None:
                break
        assert c is not None, "no seed gives the case k=%d scenario %d" % (k, scenario)
        _COLLISION_CASES[(k, scenario)] = c
    return _COLLISION_CASES[(k, scenario)]
