"""The fused pre-pass's park area (option "pp_park"): the reads of list A -- both first looks failed -- keep their codes in LDS for phases 2 and 3
instead of being written to memory and read back, and only those these phases do not finish are written out.  Pairs must equal the oracle's
at every capacity (option "debug_pp_park_cap") and segment length, the chunks of every unfinished read must be the format's
(tests.util.ref_chunks), and the parking counters must say that reads were parked, or overflowed, where they should have been."""
import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.util import chunk_offsets, cut_unitigs, random_genome, rc, ref_chunks

pytestmark = pytest.mark.gpu

FIN_PASS_DONE = 0xFFFFFFFD
PARKED, OVERFLOWED = 42, 43            # fin_batch_pipeline_counts words
GENOME_LEN = 100_000
KS = (16, 31, 32, 33, 47, 63)
PARK_CASES = [(1, None), (0, None), (1, 0), (1, 1), (1, 7), (1, 64)]   # (pp_park, debug_pp_park_cap)

_G = {}


def genome():
    if "g" not in _G:
        _G["g"] = random_genome(np.random.default_rng(4242), GENOME_LEN)
    return _G["g"]


def _sub(rng, s, lo, hi):
    """s with one substitution at a position in [lo, hi)"""
    if hi <= lo:
        return s
    i = int(rng.integers(lo, hi))
    return s[:i] + "ACGT"[("ACGT".index(s[i]) + int(rng.integers(1, 4))) % 4] + s[i + 1:]


def genome_read(rng, k, L, mode):
    """a genome read of L bases.  mode "first": an error in the first k-mer of the strand that matches (list A); "both": also in its last
    k-mer (list B); "n": a first-k-mer error and an N (list A, not all ACGT); "clean": none.  Either strand."""
    gs = genome()
    a = int(rng.integers(0, len(gs) - L))
    s = gs[a:a + L]
    if mode in ("first", "both", "n"):
        s = _sub(rng, s, 0, min(k, L))
    if mode == "both":
        s = _sub(rng, s, max(0, L - k), L)
    if mode == "n":
        i = int(rng.integers(0, L))
        s = s[:i] + "N" + s[i + 1:]
    return s if rng.random() < 0.5 else rc(s)


def mixed_reads(k):
    """lengths 31..256 in one batch: reads with errors in their first and/or last k-mers, non-ACGT reads in list A, reads from nowhere and
    clean reads"""
    rng = np.random.default_rng(500 + k)
    reads = []
    for _ in range(1500):
        L = int(rng.integers(31, 257))
        mode = ["first", "first", "both", "both", "n", "clean", "nowhere"][int(rng.integers(0, 7))]
        if mode == "nowhere":
            reads.append("".join("ACGT"[int(x)] for x in rng.integers(0, 4, L)))
        else:
            reads.append(genome_read(rng, k, L, mode))
    return reads


def overflow_reads(k):
    """1100 reads of 150 bases, each with an error in its first and in its last k-mer: whichever strand the index holds, both first looks
    fail, so every read goes to list A -- far more than a block's park area holds"""
    rng = np.random.default_rng(900 + k)
    return [genome_read(rng, k, 150, "both") for _ in range(1100)]


_IDX = {}


def index(k):
    if k not in _IDX:
        unitigs = cut_unitigs(np.random.default_rng(100 + k), genome(), k, max_len=600)
        _IDX[k] = (fa.FinimizerIndex.build(unitigs, k).to_device(0), OracleIndex.build(unitigs, k), {})
    return _IDX[k]


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for p, _, _ in _IDX.values():
        p.close()
    _IDX.clear()


def expected(k, name, reads):
    _, o, memo = index(k)
    if name not in memo:
        memo[name] = o.search_batch(reads, n_threads=8)[0]
    return memo[name]


def run(p, reads, park, cap, seg):
    opts = {"fused_ingest": 1, "pp_park": park, "debug_pp_park_cap": cap, "debug_pp_seg": seg}
    for n, v in opts.items():
        p.set_option(n, v)
    try:
        b = p.batch(reads)
        try:
            b.run(fa.FIN_MERGED)
            got, npos = b.download()
            fused, ch, pv = b.debug_ingest(int(chunk_offsets(reads)[-1]))
            pc = b.pipeline_counts(48)
        finally:
            b.close()
    finally:
        for n in opts:
            p.set_option(n, None)
    return got.astype(np.int64), npos, fused, ch, pv, pc


def check(k, name, reads, park, cap, seg):
    p, _, _ = index(k)
    got, npos, fused, ch, pv, pc = run(p, reads, park, cap, seg)
    what = (k, name, park, cap, seg)
    assert fused, what
    exp = expected(k, name, reads)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, ("pairs differ from the oracle", what, int(bad.size))
    assert npos == int((exp[:, 0] != -1).sum()), ("found count", what)
    # every read left unfinished has the format's chunks (a finished read's are undefined: nothing reads them)
    left = ~((pv[:, 0] == FIN_PASS_DONE) & (pv[:, 1] == FIN_PASS_DONE))
    off = chunk_offsets(reads)
    mask = np.repeat(left, np.diff(off))
    ref = ref_chunks(reads)
    badc = np.nonzero(mask & (ch != ref).any(axis=1))[0]
    assert badc.size == 0, ("chunks differ from the format", what, int(badc.size))
    return int(pc[PARKED]), int(pc[OVERFLOWED])


@pytest.mark.parametrize("seg", [256, 1024])
@pytest.mark.parametrize("k", KS)
def test_parked_pairs_and_chunks(k, seg):
    reads = mixed_reads(k)
    for park, cap in PARK_CASES:
        parked, _ = check(k, "mixed", reads, park, cap, seg)
        if park == 0 or cap == 0:
            assert parked == 0, (k, seg, park, cap, parked)
        else:
            assert parked > 0, (k, seg, park, cap)
            if cap is not None:
                assert parked <= cap * ((len(reads) + seg - 1) // seg), (k, seg, cap, parked)


@pytest.mark.parametrize("k", [31, 63])
def test_list_a_overflow(k):
    """a segment whose every read goes to list A: the reads beyond the park area are written out as before"""
    reads = overflow_reads(k)
    parked, over = check(k, "overflow", reads, 1, None, 1024)
    assert parked > 0 and over > 0, (parked, over)
    n_a = parked + over   # (every read is all ACGT: a place in list A below the capacity parks its read)
    assert n_a >= 0.95 * len(reads), n_a
    parked, over = check(k, "overflow", reads, 1, 7, 1024)
    assert 0 < parked <= 14 and parked + over == n_a, (parked, over, n_a)
    parked, over = check(k, "overflow", reads, 0, None, 1024)
    assert parked == 0 and over == n_a, (parked, over, n_a)
