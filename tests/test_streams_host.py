"""The inputs of tests/test_streams.py and what every product must be for them, made without a device, and the CPU guard of that file's method.

The stream tests let a missing wait show as a WRONG ANSWER, never as a fault: the batch holds read set A's results when read set B is loaded and run behind a
delay, so a call that overtakes the run reads A's pairs, records, segments, classes ... -- valid data of the same geometry.  That only works if A and B have the
same read lengths (same offsets, same buffer sizes) and different answers in every product that is compared; the guard below asserts both."""
import functools

import numpy as np

from oracle.oracle import OracleIndex, format_pairs
from tests.test_colors_host import pack_members, random_matrix, rows_of, unpack
from tests.test_read_class_host import classes_of, run_labelling, tally_of
from tests.test_read_summary_host import rule, summaries_of
from tests.test_segments_host import segments_of
from tests.test_unitig_counts import profile_of
from tests.util import cut_unitigs, random_genome, sample_reads

KS = (31, 63)          # one-word and two-word pre-pass
N_READS, READ_LEN = 600, 150
N_COLORS, ADDED_COLOR = 5, 4   # the matrix the tests upload has column ADDED_COLOR empty: Colors.add fills it


def read_set(rng, g, k, unitigs, n=N_READS):
    """n reads of READ_LEN bases: two thirds from the fast path's read mix (tests/test_search_gpu.py::_fast_path_reads -- reads inside one unitig with a few
    substitutions, either strand, and reads it must leave to the pipeline), 30 % sampled with 2 % errors (the walk kernel), the rest from nowhere (the route
    kernel fills them)"""
    from tests.test_search_gpu import _fast_path_reads
    fast = [r for r in _fast_path_reads(rng, g, k, unitigs) if len(r) == READ_LEN][: 2 * n // 3]
    nowhere = [random_genome(rng, READ_LEN) for _ in range(n // 30)]
    reads = fast + sample_reads(rng, g, n - len(fast) - len(nowhere), READ_LEN, err=0.02, random_frac=0.0) + nowhere
    assert len(reads) == n and all(len(r) == READ_LEN for r in reads)
    return [reads[i] for i in rng.permutation(n)]


class Expected:
    """every product of one read set, from the oracle's pairs and the numpy definitions of the other test files"""

    def __init__(self, o, reads, k, labels, bits):
        from tests.test_unitig_coverage import Want as CoverWant
        from tests.test_unitig_depth import Want as DepthWant
        self.reads = reads
        self.nks = np.array([max(0, len(r) - k + 1) for r in reads], dtype=np.int64)
        self.pairs = o.search_batch(reads, n_threads=8)[0][: int(self.nks.sum())]
        self.found = int((self.pairs[:, 0] != -1).sum())
        n_unitigs = len(labels)
        self.profile = profile_of(self.pairs, n_unitigs)
        self.cover, self.depth = CoverWant(self.pairs, o.ends()), DepthWant(self.pairs, o.ends())
        self.segments, self.summaries = segments_of(self.pairs, self.nks), summaries_of(self.pairs, self.nks)
        self.screen = rule(self.summaries, self.nks, 20, 300, False)
        self.classes = classes_of(self.pairs, self.nks, labels)
        self.tally = tally_of(self.classes, self.nks, int(labels[labels != 0xFFFFFFFF].max()) + 1, 1, 0, 0)
        self.rows = {pm: rows_of(self.pairs, self.nks, bits, N_COLORS, pm) for pm in (0, 1000)}
        at = np.concatenate([[0], np.cumsum(self.nks)])
        self.text = "".join(format_pairs(self.pairs[at[r]:at[r + 1]]) for r in range(len(reads))).encode()
        member = np.zeros((n_unitigs, N_COLORS), dtype=np.uint8)
        member[np.unique(self.pairs[self.pairs[:, 0] >= 0, 0]), ADDED_COLOR] = 1
        self.painted = pack_members(member)   # what Colors.add(batch, ADDED_COLOR) sets in an empty matrix
        for a in (self.pairs, self.nks, self.profile, self.classes, self.tally, self.painted):
            a.setflags(write=False)


class Case:
    def __init__(self, k):
        rng = np.random.default_rng(2800 + k)
        self.k = k
        self.genome = random_genome(rng, 40000)
        self.unitigs = cut_unitigs(rng, self.genome, k, max_len=900)
        self.oracle = OracleIndex.build(self.unitigs, k)
        n = len(self.unitigs)
        self.labels = run_labelling(rng, n)
        member = unpack(random_matrix(rng, n, N_COLORS), N_COLORS); member[:, ADDED_COLOR] = 0
        self.bits = pack_members(member)
        make = lambda reads: Expected(self.oracle, reads, k, self.labels, self.bits)
        self.A, self.B = make(read_set(rng, self.genome, k, self.unitigs)), make(read_set(rng, self.genome, k, self.unitigs))
        # scenario 7 reloads a bigger set into a batch that holds B: every buffer grows
        self.bigger = make(read_set(rng, self.genome, k, self.unitigs, n=N_READS + N_READS // 2) + [self.genome[500:900]])


@functools.lru_cache(maxsize=None)
def case(k):
    return Case(k)


def test_the_two_read_sets_have_one_geometry_and_different_answers():
    for k in KS:
        c = case(k)
        A, B = c.A, c.B
        assert [len(r) for r in A.reads] == [len(r) for r in B.reads] and len(A.reads) == N_READS
        assert np.array_equal(A.nks, B.nks) and int(A.nks.sum()) == N_READS * (READ_LEN - k + 1) == len(A.pairs) == len(B.pairs)
        differ = {
            "pairs": not np.array_equal(A.pairs, B.pairs),
            "profile": not np.array_equal(A.profile, B.profile),
            "bitmap": not np.array_equal(A.cover.bits, B.cover.bits) and not np.array_equal(A.cover.covered, B.cover.covered),
            "depth": not np.array_equal(A.depth.depth, B.depth.depth),
            "segments": A.segments[1].tobytes() != B.segments[1].tobytes() and not np.array_equal(A.segments[0], B.segments[0]),
            "summaries": A.summaries.tobytes() != B.summaries.tobytes(),
            "screen": not np.array_equal(A.screen, B.screen),
            "classes": A.classes.tobytes() != B.classes.tobytes(),
            "tally": not np.array_equal(A.tally, B.tally),
            "rows": all(not np.array_equal(A.rows[pm][0], B.rows[pm][0]) for pm in A.rows),
            "painted": not np.array_equal(A.painted, B.painted),
            "text": A.text != B.text,
        }
        assert all(differ.values()), "k=%d: A and B agree in %s" % (k, [n for n, d in differ.items() if not d])
        # sums too: an accumulator that holds A + B, 2 B or B alone are three different things
        assert A.found != B.found and not np.array_equal(A.profile + B.profile, 2 * B.profile)
        # every path takes part: reads all found (the fast path), reads partly found (the walk kernel), reads from nowhere (the route kernel's fill)
        for s in (A, B):
            f = s.summaries["n_found"].astype(np.int64)
            assert (f == s.nks).sum() > 50 and ((f > 0) & (f < s.nks)).sum() > 50 and (f == 0).sum() >= N_READS // 30
            assert 0 < s.screen.sum() < N_READS and s.painted.any() and 0 < s.tally[-1] < N_READS
        # scenario 5: colour ADDED_COLOR, painted by A's run, shows in B's rows, so rows made before the add differ from rows made behind it
        final = c.bits | A.painted
        for pm in (0, 1000):
            assert not np.array_equal(rows_of(B.pairs, B.nks, final, N_COLORS, pm)[0], B.rows[pm][0])
        assert len(c.bigger.reads) > N_READS and len(c.bigger.pairs) > len(B.pairs) and max(len(r) for r in c.bigger.reads) > READ_LEN
