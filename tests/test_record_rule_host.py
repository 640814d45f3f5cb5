"""The record gap rule at the smallest sizes where it can go wrong, exhaustively (no GPU): a position E of a kind-1 record makes strand slots [E - (k - 1), E]
absent, clamped to [0, nk - 1], and gaps may touch or overlap.  For k in {1, 2, 3, 5} and nk in 1 .. 6, EVERY strictly ascending list of at most eight positions in
[0, nk + k - 1), on both strands, is a kind-1 record inside a unitig with room for it; kind-0 and kind-2 reads lie between them so that the stream bookkeeping is
exercised.  The expectation is tests/test_records.py::brute_expand, the Python statement of the record's meaning, never a C function: fin_expand_records is held
against it, and fin_records_unitig_counts, fin_records_cover, fin_records_depth, fin_records_segments (with fin_expand_segments back) and
fin_records_read_summaries against what those pairs imply under the numpy definitions of the other host tests."""
from itertools import combinations

import numpy as np
import pytest

import finito_amd as fa
from tests.test_read_summary_host import assert_summaries, summaries_of
from tests.test_records import brute_expand
from tests.test_segments_host import assert_segments, segments_of
from tests.test_unitig_counts import profile_of
from tests.test_unitig_coverage_host import bits_of
from tests.test_unitig_depth_host import depth_of

KS = (1, 2, 3, 5)
NKS = range(1, 7)
LENS = (40, 17, 64, 23, 130)   # unitig lengths: starts 0, 40, 57, 121, 144 -- stretches cross the bitmap's word boundaries at 64, 128 and 192
# the searched reads between the records: (unitig, offset) slots, ascending and descending runs, a repeat, absent slots at either end and inside
SEARCHED = ([(2, 3), (2, 4), (-1, -1), (2, 9), (2, 8)], [(-1, -1), (4, 100), (4, 100), (0, 0)], [(1, 5)], [], [(3, 2), (3, 1), (3, 0), (-1, -1)])


def record_set(k):
    """(recs, stream, n_kind1): every position list for this k, the records in enumeration order, a kind-0 or a kind-2 read after every third of them"""
    rows, stream, i = [], [], 0
    for nk in NKS:
        m = nk + k - 1
        for nE in range(0, min(m, 8) + 1):
            for Es in combinations(range(m), nE):
                for rev in (0, 1):
                    u = i % len(LENS)
                    room = LENS[u] - k + 1 - nk   # the unitig's k-mers the record leaves free
                    off0 = (0, room, (7 * i) % (room + 1))[i % 3]
                    rows.append((u, off0, nE | (rev << 8) | (1 << 16), nk, sum(E << (16 * e) for e, E in enumerate(Es[:4])), sum(E << (16 * e) for e, E in enumerate(Es[4:]))))
                    i += 1
                    if i % 3 == 0:
                        if (i // 3) % 2:
                            s = SEARCHED[(i // 6) % len(SEARCHED)]
                            rows.append((0, 0, 0, len(s), 0, 0)); stream += s
                        else:
                            rows.append((0, 0, 2 << 16, (i // 6) % 4, 0, 0))
    recs = np.array(rows, dtype=fa.RECORD_DTYPE)
    return recs, np.array(stream, dtype=np.int32).reshape(-1, 2), i


def test_the_enumeration_is_what_it_says():
    total = 0
    for k in KS:
        recs, stream, n1 = record_set(k)
        one = recs[recs["meta"] >> 16 == 1]
        want = sum(2 * sum(len(list(combinations(range(nk + k - 1), e))) for e in range(min(nk + k - 1, 8) + 1)) for nk in NKS)
        assert len(one) == n1 == want == len(set(zip(one["nk"].tolist(), one["meta"].tolist(), one["Es"].tolist(), one["Es2"].tolist())))   # no list twice
        assert (recs["meta"] >> 16 == 0).sum() > 10 and (recs["meta"] >> 16 == 2).sum() > 10 and int(recs["nk"][recs["meta"] >> 16 == 0].sum()) == len(stream)
        total += len(recs)
    assert (recs["meta"] & 0xFF).max() == 8   # (k = 5, nk >= 4: lists of eight positions exist)
    assert total < 10 ** 4


@pytest.mark.parametrize("k", KS)
def test_every_position_list_against_the_python_definition(k):
    recs, stream, _ = record_set(k)
    ends = np.cumsum(LENS).astype(np.int64)
    nks = recs["nk"]
    want = brute_expand(recs, stream, k)
    npos = int((want[:, 0] != -1).sum())
    profile, bits, depth, segs, summ = profile_of(want, len(ends)), bits_of(want, ends)[0], depth_of(want, ends), segments_of(want, nks), summaries_of(want, nks)
    for threads in (1, 3):
        what = "k=%d threads=%d" % (k, threads)
        got, pos = fa.expand_records(recs, stream, k, n_threads=threads)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0 and pos == npos, "%s: %d pairs differ, first %d: got %s, want %s" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])
        assert np.array_equal(fa.records_unitig_counts(recs, stream, k, len(ends), n_threads=threads), profile), what
        assert np.array_equal(fa.records_cover(recs, stream, k, ends, n_threads=threads), bits), what
        assert np.array_equal(fa.records_depth(recs, stream, k, ends, n_threads=threads), depth), what
        seg = fa.records_segments(recs, stream, k, n_threads=threads)
        assert_segments(seg, segs, what)
        back, pos = fa.expand_segments(seg[0], seg[1], nks, n_threads=threads)
        assert np.array_equal(back, want) and pos == npos, what
        assert_summaries(fa.records_read_summaries(recs, stream, k, n_threads=threads), summ, what)
