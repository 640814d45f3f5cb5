"""Read ingest against an independent statement of the chunk format (tests.util.ref_chunks) and against the oracle, on reads built where
ingest goes wrong: every length from 0 to 300, runs of empty reads at the ends of a batch and across the pack kernel's 64-chunk rounds and
256-chunk wave spans, short reads whose 32-byte windows overhang into the guard bytes, and every byte value 0x00..0xFF at every position
mod 32 of a read, at its first and last k-mers and at chunk boundaries.

Both writers of chunks are checked: the pack kernel (fin_pack.hip, option fused_ingest 0) for every chunk, and the fast pre-pass's fused
ingest (fin_prepass.hip) for every read it does not finish, at k from 16 to 63, several string lengths cbf_m and both fused kernels."""
import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.util import chunk_offsets, cut_unitigs, random_genome, rc, ref_chunks, sample_reads

pytestmark = pytest.mark.gpu

FIN_PASS_DONE = 0xFFFFFFFD
GENOME_LEN = 120_000
NOT_BASES = bytes(b for b in range(256) if (b & 0xDF) not in b"ACGT")


# ---- read sets ---------------------------------------------------------------------------------------------------------------------------
def _piece(rng, gs, n):
    """n bases of the genome, either strand"""
    a = int(rng.integers(0, len(gs) - n + 1))
    s = gs[a:a + n]
    return (s if rng.random() < 0.5 else rc(s)).encode()


def _junk(rng, n):
    return bytes(NOT_BASES[int(x)] for x in rng.integers(0, len(NOT_BASES), n))


class _Reads:
    """a read list that knows its chunk offset"""

    def __init__(self):
        self.reads, self.off = [], 0

    def add(self, r):
        self.reads.append(r)
        self.off += 2 * ((len(r) + 31) // 32)

    def pad_to(self, rng, gs, target, max_len):
        """genome reads until the next read's first chunk is `target` (chunk offsets are even: 1-base reads close the gap)"""
        assert target % 2 == 0 and target >= self.off
        while target - self.off > 2:
            n = int(rng.integers(1, max_len + 1))
            if self.off + 2 * ((n + 31) // 32) > target - 2:
                n = 32 * ((target - 2 - self.off) // 2) if target - 2 - self.off >= 2 else 0
                if n == 0:
                    break
            self.add(_piece(rng, gs, n))
        while self.off < target:
            self.add(_piece(rng, gs, 1))
        assert self.off == target


def geometry_batch(rng, gs, max_len=300):
    """every length 0..max_len; runs of 1, 63, 64, 65, 200 empty reads at the start, the end, and two chunks before, at and after multiples of
    64 and 256 chunks; reads that start or end at a 256-chunk boundary or straddle one; a stretch of 1-base reads"""
    b = _Reads()
    for _ in range(200):
        b.add(b"")
    b.add(_piece(rng, gs, 5))
    for n in range(max_len + 1):
        b.add(_piece(rng, gs, n))
        if n % 37 == 0:
            b.add(_piece(rng, gs, 1))
    for _ in range(300):
        b.add(_piece(rng, gs, 1))
    for run in (1, 63, 64, 65, 200):
        for unit in (64, 256):
            for d in (-2, 0, 2):
                target = (b.off // unit + 1) * unit + d
                if target < b.off:
                    target += unit
                b.pad_to(rng, gs, target, max_len)
                for _ in range(run):
                    b.add(b"")
        # a read across a span boundary, and one that starts right at it
        b.pad_to(rng, gs, (b.off // 256 + 1) * 256 - 4, max_len)
        b.add(_piece(rng, gs, max_len))
        b.pad_to(rng, gs, (b.off // 256 + 1) * 256, max_len)
        b.add(_piece(rng, gs, 64))
    b.add(_piece(rng, gs, 3))
    for _ in range(63):
        b.add(b"")
    return b.reads


def sized_batch(rng, gs, n_reads, max_len=300):
    """n_reads reads, short ones (1..31 bases) first and last: their windows overhang into the guard bytes in front of and behind the batch"""
    if n_reads == 1:
        return [_piece(rng, gs, 17)]
    mid = []
    for i in range(n_reads - 2):
        t = i % 11
        mid.append(b"" if t in (3, 4, 5) else _piece(rng, gs, int(rng.integers(1, 32)) if t == 7 else int(rng.integers(1, max_len + 1))))
    return [_piece(rng, gs, int(rng.integers(1, 32)))] + mid + [_piece(rng, gs, int(rng.integers(1, 32)))]


def alphabet_batch(rng, gs, k, max_len=256):
    """every byte value at every position mod 32, at the strands' first and last k-mers, the middle, chunk boundaries 31/32/63/64, k-1 and
    len-k; reads of no base at all; reads whose only stretch of bases is shorter than k; clean reads beside junk-filled ones"""
    reads = []

    def with_bytes(L, put):
        s = bytearray(_piece(rng, gs, L))
        for p, v in put:
            s[p] = v
        return bytes(s)

    # every (byte, position mod 32), two per read of 150 bases: positions p + 32 t, t = 0..3
    combos = [(v, p) for v in range(256) for p in range(32)]
    order = rng.permutation(len(combos))
    for i in range(0, len(order), 2):
        (v1, p1), (v2, p2) = combos[order[i]], combos[order[i + 1]]
        t1 = int(rng.integers(0, 4))
        t2 = (t1 + 1 + int(rng.integers(0, 3))) % 4
        reads.append(with_bytes(150, [(p1 + 32 * t1, v1), (p2 + 32 * t2, v2)]))
    # every byte at the places where a mask or a cut-off goes wrong: one near each end of a read
    pairs = [(0, -1), (k - 1, -k), (k - 2, -k - 1), (k, -k + 1), (31, 64), (32, 63), (1, None), (None, -2)]
    lens = [k, k + 1, 64, 65, 96, 150, 200, max_len]
    for v in range(256):
        for j, (a, e) in enumerate(pairs):
            L = lens[(v + j) % len(lens)]
            put = []
            for p in (a, e):
                if p is not None:
                    p = p if p >= 0 else L + p
                    if 0 <= p < L:
                        put.append((p, v))
            reads.append(with_bytes(L, put))
        M = int(rng.integers(k, max_len + 1))
        reads.append(with_bytes(M, [(M // 2, v)]))
    # no base at all; a stretch of bases shorter than k (or exactly k) between junk; clean reads right beside junk-filled ones
    for n in list(range(1, 40)) + [63, 64, 65, 128, 200, max_len]:
        reads.append(_junk(rng, n))
        reads.append(_piece(rng, gs, int(rng.integers(k, max_len + 1))))
        reads.append(NOT_BASES[n % len(NOT_BASES):][:1] * n)
        reads.append(_piece(rng, gs, int(rng.integers(1, 32))))
    for m in (1, k - 2, k - 1, k):
        for lead in (0, 1, 7, 31, 32, 33):
            reads.append(_junk(rng, lead) + _piece(rng, gs, m) + _junk(rng, int(rng.integers(0, 40))))
            reads.append(_piece(rng, gs, int(rng.integers(k, max_len + 1))))
    # lower case, whole and in part
    for _ in range(20):
        s = _piece(rng, gs, int(rng.integers(k, max_len + 1)))
        a = int(rng.integers(0, len(s)))
        reads.append(s.lower() if rng.random() < 0.3 else s[:a] + s[a:].lower())
    return reads


# ---- indexes and runs ------------------------------------------------------------------------------------------------------------------
_GENOME = {}


def genome():
    if not _GENOME:
        _GENOME["g"] = random_genome(np.random.default_rng(2024), GENOME_LEN)
    return _GENOME["g"]


def _index(k, cbf_m=None, lean=None):
    rng = np.random.default_rng(1000 + k)
    unitigs = cut_unitigs(rng, genome(), k, max_len=600)
    p = fa.FinimizerIndex.build(unitigs, k)
    if cbf_m is not None:
        p.set_option("cbf_m", cbf_m)
    if lean is not None:
        p.set_option("lean_tables", lean)
    return p.to_device(0), unitigs


_ORACLES = {}


def oracle(k):
    if k not in _ORACLES:
        rng = np.random.default_rng(1000 + k)
        _ORACLES[k] = OracleIndex.build(cut_unitigs(rng, genome(), k, max_len=600), k)
    return _ORACLES[k]


_FUSED_READS = {}


def fused_reads(k):
    """geometry + alphabet + genome reads with sequencing errors on both strands, all at most 256 bases (the fused ingest's limit); the
    genome reads' indices"""
    if k not in _FUSED_READS:
        rng = np.random.default_rng(3000 + k)
        gs = genome()
        reads = geometry_batch(rng, gs, max_len=256) + alphabet_batch(rng, gs, k)
        n0 = len(reads)
        for L in (100, 150, 256):
            reads += [r.encode() for r in sample_reads(rng, gs, 800, L, err=0.01, random_frac=0.03)]
        _FUSED_READS[k] = (reads, np.arange(n0, len(reads)))
    return _FUSED_READS[k]


_MEMO = {}


def _memo(kind, reads, fn):
    key = (kind, id(reads))
    if key not in _MEMO:
        _MEMO[key] = (reads, fn())   # (keeps the list alive: its id stays its own)
    return _MEMO[key][1]


def expected(o, reads):
    return _memo(("oracle", o.k), reads, lambda: o.search_batch(reads, n_threads=8)[0])


def run_batch(p, reads, strands=fa.FIN_MERGED):
    """pairs, found count, (fused, chunks, verdicts) of the run, run_info"""
    b = p.batch(reads)
    try:
        b.run(strands)
        got, npos = b.download()
        fused, ch, pv = b.debug_ingest(int(chunk_offsets(reads)[-1]))
        info = b.run_info()
    finally:
        b.close()
    return got.astype(np.int64), npos, (fused, ch, pv), info


def assert_pairs(got, npos, exp, what):
    assert got.shape == exp.shape, what
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, ("pairs differ from the oracle", what, int(bad.size), int(bad[0]))
    assert npos == int((exp[:, 0] != -1).sum()), ("found count", what)


def assert_chunks(ch, reads, which, what):
    """the chunks of the reads `which` (bool per read) equal ref_chunks byte for byte"""
    ref = _memo("ref", reads, lambda: ref_chunks(reads))
    off = chunk_offsets(reads)
    mask = np.repeat(which, np.diff(off))
    bad = np.nonzero(mask & (ch != ref).any(axis=1))[0]
    if bad.size:
        r = int(np.searchsorted(off, bad[0], side="right") - 1)
        raise AssertionError(("chunks differ from the format", what, int(bad.size), "read", r, reads[r], "chunk", int(bad[0] - off[r]),
                              ch[bad[0]].tolist(), ref[bad[0]].tolist()))
    return int(which.sum())


@pytest.fixture(scope="module")
def k31():
    p, _ = _index(31)
    yield p, oracle(31)
    p.close()


def _batches31():
    rng = np.random.default_rng(77)
    gs = genome()
    out = [("geometry", geometry_batch(rng, gs)), ("alphabet", alphabet_batch(rng, gs, 31))]
    out += [("n%d" % n, sized_batch(rng, gs, n)) for n in (1, 255, 256, 257, 1025)]
    return out


@pytest.fixture(scope="module")
def batches31():
    return _batches31()


# ---- the pack kernel -------------------------------------------------------------------------------------------------------------------
def test_pack_kernel_chunks_are_the_format(k31, batches31):
    """kernel 4 without the fused ingest: the pack kernel writes every chunk of the batch, each one the format's"""
    p, o = k31
    p.set_option("fused_ingest", 0)
    try:
        for name, reads in batches31:
            got, npos, (fused, ch, _), info = run_batch(p, reads)
            assert info["kernel"] == 4 and not fused, (name, info)
            assert_chunks(ch, reads, np.ones(len(reads), dtype=bool), name)
            assert_pairs(got, npos, expected(o, reads), name)
    finally:
        p.set_option("fused_ingest", None)


# ---- the fused ingest ------------------------------------------------------------------------------------------------------------------
def check_fused(p, o, reads, sampled, what, min_done):
    p.set_option("fused_ingest", 1)
    try:
        got, npos, (fused, ch, pv), info = run_batch(p, reads)
    finally:
        p.set_option("fused_ingest", None)
    assert fused and info["kernel"] == 4 and info["fast_path"], (what, fused, info)
    assert_pairs(got, npos, expected(o, reads), what)
    done = (pv[:, 0] == FIN_PASS_DONE) & (pv[:, 1] == FIN_PASS_DONE)
    n = assert_chunks(ch, reads, ~done, what)   # (a read the fast path finished has no chunks: nothing reads them)
    assert n > 0, what
    if len(sampled):
        share = float(done[sampled].mean())
        assert share >= min_done, ("the fast path finished too few reads", what, share)


# lean_tables at upload picks the fused kernel (pp_fast_kernel, fin_prepass.hip): with lean tables (the string filter fbf) and k <= 32 the
# fast kernel, fin_fast_prepass_fused_kernel (1); at k >= 33, or without lean tables (lean_tables 0 at k = 31), the fast2 kernel,
# fin_fast2_prepass_fused_kernel (2).  Both fuse the ingest at k <= 63.
FUSED_CASES = []
for _k in (16, 21, 31, 32, 33, 47, 62, 63):
    for _m in (None, 7, 13, min(_k, 32)):
        FUSED_CASES.append((_k, _m, None))
FUSED_CASES += [(31, None, 0), (31, 13, 0), (31, None, 2)]


@pytest.mark.parametrize("k,cbf_m,lean", FUSED_CASES, ids=["k%d-m%s-lean%s" % (k, m, l) for k, m, l in FUSED_CASES])
def test_fused_ingest_against_the_format(k, cbf_m, lean):
    p, _ = _index(k, cbf_m, lean)
    try:
        assert p.kmer_table_bytes() > 0 and p.string_filter_bytes() > 0
        if lean == 0:
            assert not p.lean_tables()     # -> the fast2 fused kernel at k = 31
        else:
            assert p.lean_tables()         # default 2 (k <= 63): at k <= 32 the fast fused kernel, else the fast2 one
        reads, sampled = fused_reads(k)
        # (measured on these reads: the fast path finishes 14-20 % of the genome reads with strings of 7 bases or of k-3 .. k bases, and 44-62 %
        #  at the default length and at 13 <= m <= k - 8)
        strong = cbf_m is None or 13 <= cbf_m <= k - 8
        check_fused(p, oracle(k), reads, sampled, (k, cbf_m, lean), min_done=0.35 if strong else 0.1)
    finally:
        p.close()


@pytest.mark.parametrize("seg", [256, 1024])
def test_fused_ingest_pre_pass_segments(k31, batches31, seg):
    p, o = k31
    reads, sampled = fused_reads(31)
    p.set_option("debug_pp_seg", seg)
    try:
        check_fused(p, o, reads, sampled, ("seg", seg), min_done=0.35)
        for name, rs in batches31:
            check_fused(p, o, [r[:256] for r in rs], np.arange(0), (name, seg), min_done=0.0)
    finally:
        p.set_option("debug_pp_seg", None)


def test_fused_ingest_sized_batches(k31, batches31):
    p, o = k31
    for name, reads in batches31:
        capped = [r[:256] for r in reads]
        check_fused(p, o, capped, np.arange(0), name, min_done=0.0)


def test_a_257_base_read_turns_the_fusion_off(k31):
    p, o = k31
    rng = np.random.default_rng(91)
    reads = alphabet_batch(rng, genome(), 31) + [_piece(rng, genome(), 257)]
    p.set_option("fused_ingest", 1)
    try:
        got, npos, (fused, ch, _), info = run_batch(p, reads)
    finally:
        p.set_option("fused_ingest", None)
    assert not fused and info["kernel"] == 4, info
    assert_pairs(got, npos, expected(o, reads), "257")
    assert_chunks(ch, reads, np.ones(len(reads), dtype=bool), "257")


# ---- every kernel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [4, 3, 2, 0])
def test_every_kernel_on_the_edge_batches(k31, batches31, kernel):
    """kernel 0 decodes the ASCII itself (d_base_code); the others read the chunks.  Merged and forward-only pairs"""
    p, o = k31
    p.set_option("kernel", kernel)
    try:
        for name, reads in batches31:
            got, npos, _, info = run_batch(p, reads, fa.FIN_MERGED)
            assert info["kernel"] == kernel, (name, info)
            assert_pairs(got, npos, expected(o, reads), (name, kernel, "merged"))
            got, _, _, _ = run_batch(p, reads, fa.FIN_FWD)
            exp = np.array([x for r in reads for x in o.search(r)[0]], dtype=np.int64).reshape(-1, 2)
            assert got.shape == exp.shape and np.array_equal(got, exp), (name, kernel, "forward-only")
    finally:
        p.set_option("kernel", None)


# ---- sub-batches -----------------------------------------------------------------------------------------------------------------------
def test_sub_batch_seams_inside_runs_of_empty_reads(k31, batches31):
    """fin_search_batch's pipeline with sub-batches of 3000 k-mers: their seams fall inside the runs of empty reads"""
    p, o = k31
    reads = dict(batches31)["geometry"]
    p.set_option("pipeline_kmers", 3000)
    try:
        got, npos = p.search_reads(reads, fa.FIN_MERGED)
    finally:
        p.set_option("pipeline_kmers", None)
    assert_pairs(got.astype(np.int64), npos, expected(o, reads), "sub-batches")
