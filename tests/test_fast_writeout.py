"""The fast pre-pass's write-out of the reads it finishes (option "pp_wide_out"): 1 = the read's own lane makes a gap mask over the read's output
slots once and the wave writes two neighbouring slots per lane with one 16-byte store (8 bytes at an odd first pair and at an odd end); 0 = slot
by slot, 8 bytes per lane.  Both must give the oracle's pairs, in the fused and the unfused kernels and at both segment lengths, on reads cut from
known places of a few disjoint unitigs: every alignment of a read's first pair, slot counts at the mask's word boundaries, gaps clamped at both
ends of a read and merged, on both strands -- and finished reads between unfinished ones, whose slots other kernels write: a stray store shows."""
import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import LazyCounters, OracleIndex
from tests.util import random_genome, rc

pytestmark = pytest.mark.gpu

KS = (16, 31, 33, 63)
FAST_DONE = 4 * 8 + 9                      # fin_batch_pipeline_counts word: reads finished by the fast path
MAX_LEN = 256                              # the longest read the fast path takes (FIN_FAST_CHUNKS * 32)
UNITIG_LENS = (300, 517, 1000, 1501, 2048, 3000, 777, 2600)
MIN_FAST_FRACTION = 0.6


def unitigs():
    """a few unitigs of 300 to 3000 random bases: disjoint (no k-mer of 16 or more bases occurs twice in 12 000 random bases; the test checks it)"""
    rng = np.random.default_rng(1313)
    return [random_genome(rng, n) for n in UNITIG_LENS]


def _sub(s, *positions):
    """s with a substitution at each of the positions (of the read as given: its own strand)"""
    t = list(s)
    for p in positions:
        if 0 <= p < len(t):
            t[p] = "ACGT"[("ACGT".index(s[p]) + 1 + (p % 3)) % 4]
    return "".join(t)


def make_reads(k):
    """(reads, n_triples): the batch, and how many [crossing, finished, crossing] triples lie at its end"""
    rng = np.random.default_rng(7000 + k)
    us = unitigs()

    def cut(L, strand):
        """L bases from a random place of a unitig that holds them, on the given strand"""
        u = us[int(rng.choice([i for i, x in enumerate(us) if len(x) >= L]))]
        a = int(rng.integers(0, len(u) - L + 1))
        s = u[a:a + L]
        return rc(s) if strand else s

    def crossing(L):
        """the end of one unitig and the start of another: never finished by the fast path"""
        i, j = (int(x) for x in rng.choice(len(us), 2, replace=False))
        x = int(rng.integers(k, L - k + 1))                                  # (a k-mer on either side: a look finds one, and the attempt meets the unitig's end)
        s = us[i][len(us[i]) - x:] + us[j][:L - x]
        return rc(s) if rng.random() < 0.5 else s

    lens = [k, k + 1, k + 2, 61, 62, 149, 150, 151, 255, 256]
    nks = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, MAX_LEN - k + 1]
    nk_lens = sorted({nk + k - 1 for nk in nks if nk + k - 1 <= MAX_LEN})
    reads = []
    for strand in (0, 1):
        for L in lens + nk_lens:
            reads.append(cut(L, strand))                                   # clean: every slot a pair
            if L >= k:
                reads.append(_sub(cut(L, strand), L // 2))                 # one gap in the middle (clamped at both ends in a short read)
        for L in (150, 151, 256, 2 * k + 3, k + 2):
            if L > MAX_LEN:
                continue
            for p in (0, k - 2, k - 1, k, L - k, L - 1):                   # gaps clamped at the read's ends; first or last k-mer lost: phases 2 and 3
                reads.append(_sub(cut(L, strand), p))
            reads.append(_sub(cut(L, strand), 0, L - 1))
            for p in (0, 1, L // 3, L - k - 2, L - 2):
                reads.append(_sub(cut(L, strand), p, p + 1))               # adjacent
                reads.append(_sub(cut(L, strand), p, p + k - 1))           # their gaps touch
                reads.append(_sub(cut(L, strand), p, p + k))               # ... and leave one slot open between them
            reads.append(_sub(cut(L, strand), 3, L // 3, L // 2, L - 5))   # four in one read
            reads.append(_sub(cut(L, strand), k, k + 1, 2 * k, 2 * k + 1))
    for L in (k, 62, 150, 151, 255, 256):                                  # reads from nowhere: every slot (-1,-1)
        reads.append(random_genome(rng, L))
    for _ in range(250):                                                   # several waves and blocks of ordinary reads, a substitution in most
        L = int(rng.integers(k, MAX_LEN + 1))
        s = cut(L, int(rng.integers(0, 2)))
        for _ in range(int(rng.integers(0, 4))):
            s = _sub(s, int(rng.integers(0, L)))
        reads.append(s)
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    # a finished read between two unfinished ones: the neighbours' slots come from other kernels
    n_triples = 0
    for L in (150, 151, 256, 255, 149):
        for strand in (0, 1):
            reads += [crossing(L), _sub(cut(L, strand), L // 2), crossing(L - 1)]
            n_triples += 1
    return reads, n_triples


_IDX = {}


def case(k):
    """index on the device, the oracle's pairs, the reads -- made once per k"""
    if k not in _IDX:
        us = unitigs()
        reads, n_triples = make_reads(k)
        o = OracleIndex.build(us, k)
        exp = o.search_batch(reads, n_threads=8)[0]
        lc = LazyCounters()
        lazy = o.search_batch_lazy(reads, fast=True, counters=lc, n_threads=1)
        assert np.array_equal(lazy, exp), k
        _IDX[k] = (fa.FinimizerIndex.build(us, k).to_device(0), exp, reads, n_triples, int(lc.fast_reads))
    return _IDX[k]


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for c in _IDX.values():
        c[0].close()
    _IDX.clear()


def run(p, reads, opts):
    for n, v in opts.items():
        p.set_option(n, v)
    try:
        b = p.batch(reads)
        try:
            b.run(fa.FIN_MERGED)
            got, npos = b.download()
            pc = b.pipeline_counts(48)
        finally:
            b.close()
    finally:
        for n in opts:
            p.set_option(n, None)
    return got.astype(np.int64), npos, int(pc[FAST_DONE])


def test_read_set_is_what_it_should_be():
    """the set's own conditions: disjoint unitigs; odd and even first pairs and slot counts; the lazy oracle's fast path finishes most reads"""
    for k in KS:
        us = unitigs()
        kmers = [s[i:i + k] for u in us for s in (u, rc(u)) for i in range(len(s) - k + 1)]
        assert len(set(kmers)) == len(kmers), k
        _, _, reads, _, lazy_fast = case(k)
        nk = np.array([max(0, len(r) - k + 1) for r in reads])
        first = np.concatenate(([0], np.cumsum(nk)[:-1]))
        odd = int(((first & 1) == 1).sum())
        assert 0.3 * len(reads) < odd < 0.7 * len(reads), (k, odd, len(reads))
        assert {1, 2, 63, 64, 65, 127, 128, 129, MAX_LEN - k + 1} <= set(nk.tolist()), k
        assert lazy_fast >= MIN_FAST_FRACTION * len(reads), (k, lazy_fast, len(reads))


@pytest.mark.parametrize("seg", [256, 1024])
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("k", KS)
def test_pairs_equal_the_oracle(k, fused, seg):
    p, exp, reads, n_triples, _ = case(k)
    for wide in (0, 1):
        what = (k, fused, seg, wide)
        got, npos, fast_done = run(p, reads, {"fused_ingest": fused, "debug_pp_seg": seg, "pp_wide_out": wide})
        assert fast_done >= MIN_FAST_FRACTION * len(reads), ("too few reads reach the write-out", what, fast_done, len(reads))
        assert fast_done <= len(reads) - 2 * n_triples, ("a read that crosses a unitig end was finished", what, fast_done)
        assert got.shape == exp.shape, what
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, ("pairs differ from the oracle", what, int(bad.size), bad[:8].tolist(), got[bad[:4]].tolist(), exp[bad[:4]].tolist())
        assert npos == int((exp[:, 0] != -1).sum()), ("found count", what)
