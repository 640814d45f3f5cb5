"""The enumerated digit case (tests/util.py::digit_case), the parts that need no GPU: a guard on the generator -- fin_text.hip's record-derived text has a closed
form for a read's length (digit_sum), two shared strings for the leading digits of a group's offsets (H0 = B / 1000, H1 = H0 + 1, chosen by a carry), a write
loop specialised by the unitig's digit count (4 to 7; a generic one for 1 to 3 and 8 to 10) and a staging buffer sized for 128 pairs of 24 bytes, and
tests/test_record_digits.py means something only if the case enters every one of them -- and the host functions over the same records.

Every condition is counted on the records, on tests/test_records.py::brute_expand's pairs and on the expected text's lengths (tests/util.py::pair_text_len),
never on anything the library computes."""
import numpy as np

import finito_amd as fa
from oracle.oracle import format_pairs
from tests.test_read_summary_host import assert_summaries, summaries_of
from tests.test_records import brute_expand
from tests.test_records_host import positions_of
from tests.test_segments_host import assert_segments, segments_of
from tests.util import (DIGIT_BOUNDARIES, DIGIT_H_GAINS, DIGIT_LONG, DIGIT_LONG_UNITIG, DIGIT_MAX_READS, DIGIT_NES, DIGIT_NKS, DIGIT_RUN, DIGIT_RUN_UNITIG, INT32_MAX,
                        digit_case, pair_text_len)

GROUP = 128          # pairs the record-derived text formats at a time (FIN_TEXT3_GROUP)
MAX_PAIR = 24        # "(2147483647,2147483647)" and its separator


def ndigits(v):
    return len(str(int(v)))


def text_of(pairs, nks):
    at = np.concatenate([[0], np.cumsum(nks)])
    return "".join(format_pairs(pairs[at[r]:at[r + 1]]) for r in range(len(nks))).encode()


def assert_text(got, want, what):
    """exact equality; a failure names the first differing byte with what stands around it"""
    if got != want:
        i = next((j for j, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
        raise AssertionError("%s: text of %d bytes, expected %d; first difference at byte %d (line %d): got %r, want %r" %
                             (what, len(got), len(want), i, want[:i].count(b"\n"), got[max(0, i - 40):i + 40], want[max(0, i - 40):i + 40]))


_EXPECTED = {}


def expected():
    """what every consumer must deliver for the digit case, from the pairs alone: text, found, segments, summaries.  Made once and shared"""
    if not _EXPECTED:
        c = digit_case()
        _EXPECTED.update(text=text_of(c.pairs, c.nks), found=int((c.pairs[:, 0] != -1).sum()), segments=segments_of(c.pairs, c.nks),
                         summaries=summaries_of(c.pairs, c.nks))
    return _EXPECTED


def facts():
    """per read: kind, strand, number of positions, first pair; per kind-1 read the found mask in the order of strand A's slots (slot s has offset off0 + s)"""
    c = digit_case()
    kind, nE, rev = c.recs["meta"] >> 16, c.recs["meta"] & 0xFF, (c.recs["meta"] >> 8) & 1
    at = np.concatenate([[0], np.cumsum(c.nks)])
    found = {}
    for r in np.nonzero(kind == 1)[0]:
        f = c.pairs[at[r]:at[r + 1], 0] != -1
        found[int(r)] = f[::-1] if rev[r] else f
    return c, kind, nE, rev, at, found


def test_every_digit_count_of_the_unitig_number_on_either_strand():
    c, kind, nE, rev, at, found = facts()
    for n in range(1, 11):
        for s in (0, 1):
            reads = [r for r, f in found.items() if rev[r] == s and ndigits(c.recs["u"][r]) == n and f.any()]
            assert len(reads) >= 20, "%d finished reads with a unitig number of %d digits on strand %d" % (len(reads), n, s)
            # the write loop's specialisation meets every way the offset's leading digits behave: no H, a carry into an H of the same length, a longer H + 1
            gains = {P for r in reads for P in (1000 * (H + 1) for H in DIGIT_H_GAINS) if c.recs["off0"][r] < P <= c.recs["off0"][r] + c.nks[r] - 1}
            assert len(gains) >= 3, "%d digits, strand %d: reads across %s only" % (n, s, sorted(gains))
    assert (c.recs["u"].astype(np.int64) <= INT32_MAX).all() and (c.recs["off0"].astype(np.int64) + c.nks - 1 <= INT32_MAX)[kind == 1].all()
    for nk in DIGIT_NKS:
        for s in (0, 1):
            assert ((kind == 1) & (c.nks == nk) & (rev == s)).sum() >= 20, (nk, s)
    for e in DIGIT_NES:
        for s in (0, 1):
            assert ((kind == 1) & (nE == e) & (rev == s)).sum() >= 100, (e, s)
    assert set(int(x) for x in nE[kind == 1]) == set(DIGIT_NES) and (c.recs["Es2"][(kind == 1) & (nE == 8)] >> 48 != 0).sum() >= 100


def test_every_boundary_is_crossed_and_is_gapped():
    """per boundary P and strand: a read with found pairs at P - 1 and at P (2^31: at P - 1, its last slot); per boundary: a read whose slot at P - 1 or P lies in a
    gap, one whose gap ends on the slot in front of a found P - 1 or P, and gaps clamped at slot 0 and at nk - 1"""
    c, kind, nE, rev, at, found = facts()
    k = c.k
    for P in DIGIT_BOUNDARIES:
        crossed, gapped, behind = {0: 0, 1: 0}, 0, 0
        for r, f in found.items():
            off0, nk = int(c.recs["off0"][r]), int(c.nks[r])
            a, b = P - 1 - off0, P - off0
            if 0 <= a < nk and f[a] and (P > INT32_MAX or (b < nk and f[b])):
                crossed[int(rev[r])] += 1
            gapped += any(0 <= s < nk and not f[s] for s in (a, b))
            behind += any(1 <= s < nk and f[s] and not f[s - 1] for s in (a, b))
        assert crossed[0] >= 3 and crossed[1] >= 3, "boundary %d is crossed by %s reads" % (P, crossed)
        assert gapped >= 1 and (behind >= 1 or P == 2 ** 31), "boundary %d: %d reads with the slot in a gap, %d with a gap that ends in front of it" % (P, gapped, behind)
    # offsets below 1000: reads that start at 0 and reads that end on a number of one, two and three digits
    ends_on = {int(c.recs["off0"][r]) + int(c.nks[r]) - 1 for r, f in found.items() if f[-1]}
    assert {9, 10, 99, 100, 999} <= ends_on and sum(1 for r, f in found.items() if c.recs["off0"][r] == 0 and f[0]) >= 10
    clamp0 = sum(1 for r in found if any(E < k - 1 for E in positions_of(c.recs[r])))
    clamp_end = sum(1 for r in found if any(E >= c.nks[r] for E in positions_of(c.recs[r])))
    whole = sum(1 for r, f in found.items() if nE[r] and not f.any())
    assert clamp0 >= 50 and clamp_end >= 50 and whole >= 5, (clamp0, clamp_end, whole)


def group_starts(c, at, reads):
    """(byte offset in the expected text, bytes) of every group of GROUP pairs of the given reads"""
    first_byte = np.concatenate([[0], np.cumsum(pair_text_len(c.pairs))])
    out = []
    for r in reads:
        for i0 in range(int(at[r]), int(at[r + 1]), GROUP):
            out.append((int(first_byte[i0]), int(first_byte[min(i0 + GROUP, int(at[r + 1]))] - first_byte[i0])))
    return out


def test_alignments_and_lengths_of_the_groups():
    """the staging buffer holds GROUP * MAX_PAIR bytes at the text's own offset modulo 16: every offset occurs, for finished and for searched reads, and a group of
    GROUP * MAX_PAIR bytes occurs at every one of them -- 15 + 3072 bytes is the most a wave ever stages"""
    c, kind, nE, rev, at, found = facts()
    assert int(pair_text_len(c.pairs).max()) == MAX_PAIR
    for name, reads in (("finished", np.nonzero(kind == 1)[0]), ("searched", np.nonzero(kind == 0)[0])):
        groups = group_starts(c, at, reads)
        assert {a % 16 for a, _ in groups} == set(range(16)), "%s reads: groups start at %s modulo 16" % (name, sorted({a % 16 for a, _ in groups}))
        full = [a % 16 for a, n in groups if n == GROUP * MAX_PAIR]
        assert max(n for _, n in groups) == GROUP * MAX_PAIR and set(full) == set(range(16)), "%s reads: full groups at %s modulo 16" % (name, sorted(set(full)))
    every = c.pairs[np.repeat(kind == 0, c.nks)]
    longest = [r for r in np.nonzero(kind == 0)[0] if c.nks[r] >= 260 and (c.pairs[at[r]:at[r + 1]] == INT32_MAX).all()]
    assert len(longest) == DIGIT_MAX_READS >= 3
    for col in (0, 1):   # the searched reads' numbers: every digit count in both fields, and absent pairs
        assert {ndigits(v) for v in every[every[:, 0] >= 0][:, col]} == set(range(1, 11))
    assert (every[:, 0] == -1).sum() > 1000


def test_the_records_are_legal_and_laid_out_as_stated():
    """what fin_batch_set_records asks of a record, restated; all three kinds and several digit counts in every wave of 64 reads; the run on one 6-digit unitig;
    the four long reads"""
    c, kind, nE, rev, at, found = facts()
    k = c.k
    assert set(int(x) for x in kind) == {0, 1, 2} and (c.nks >= 1).all() and len(c.reads) == len(c.recs)
    assert all(len(r) == nk + k - 1 for r, nk in zip(c.reads, c.nks)) and max(len(c.reads[r]) for r in found if c.nks[r] < 4000) == 300
    for r in found:
        E = positions_of(c.recs[r])
        assert len(E) <= 8 and E == sorted(E) and all(x < int(c.nks[r]) + k - 1 for x in E), "record %d" % r
        assert int(c.recs["Es"][r]) >> (16 * min(len(E), 4)) == 0 and int(c.recs["Es2"][r]) >> (16 * max(len(E) - 4, 0)) == 0 and int(c.recs["meta"][r]) >> 9 == 1 << 7
    other = c.recs[kind != 1]
    assert (other["u"] == 0).all() and (other["off0"] == 0).all() and (other["Es"] == 0).all() and (other["Es2"] == 0).all() and (other["meta"] & 0xFFFF == 0).all()
    assert np.array_equal(c.pairs, brute_expand(c.recs, c.stream, k)) and c.pairs.dtype == np.int32
    run = range(*DIGIT_RUN)
    for w in range(0, len(c.recs), 64):
        if w in run:
            continue
        assert set(int(x) for x in kind[w:w + 64]) == {0, 1, 2}, "wave at read %d" % w
        assert len({ndigits(c.recs["u"][r]) for r in range(w, w + 64) if kind[r] == 1}) >= 5, "wave at read %d" % w
    assert len(run) == 256 and (kind[run.start:run.stop] == 1).all() and set(int(x) for x in c.recs["u"][run.start:run.stop]) == {DIGIT_RUN_UNITIG}
    assert ndigits(DIGIT_RUN_UNITIG) == 6 and len(set(int(x) for x in c.recs["off0"][run.start:run.stop] // 1000)) >= 5
    long = [r for r in found if c.nks[r] > 4096]
    assert sorted((int(c.nks[r]), int(rev[r])) for r in long) == sorted((nk, s) for nk, s, _ in DIGIT_LONG) == [(4097, 0), (4097, 1), (9001, 0), (9001, 1)]
    for r in long:
        off0, f = int(c.recs["off0"][r]), found[r]
        P = [P for P in (10 ** 6, 10 ** 9) if off0 < P <= off0 + int(c.nks[r]) - 1]
        assert c.recs["u"][r] == DIGIT_LONG_UNITIG and ndigits(DIGIT_LONG_UNITIG) == 10 and len(P) == 1
        assert f[:P[0] - off0 - 2 * k].any() and f[P[0] - off0 + 2 * k:].any() and f[4096:].any()


def test_host_functions_on_the_digit_case():
    """fin_expand_records, fin_records_segments, fin_expand_segments, fin_records_read_summaries and the host text formatter over the records the device is given"""
    c, e = digit_case(), expected()
    for threads in (1, 3):
        got, npos = fa.expand_records(c.recs, c.stream, c.k, n_threads=threads)
        assert np.array_equal(got, c.pairs) and npos == e["found"]
        segs = fa.records_segments(c.recs, c.stream, c.k, n_threads=threads)
        assert_segments(segs, e["segments"], "threads=%d" % threads)
        back, pos = fa.expand_segments(segs[0], segs[1], c.nks, n_threads=threads)
        assert np.array_equal(back, c.pairs) and pos == e["found"]
        assert_summaries(fa.records_read_summaries(c.recs, c.stream, c.k, n_threads=threads), e["summaries"], "threads=%d" % threads)
    at = np.concatenate([[0], np.cumsum(c.nks)])
    assert_text("".join(fa.format_pairs(c.pairs[at[r]:at[r + 1]]) for r in range(len(c.nks))).encode(), e["text"], "the host formatter")
    assert len(e["text"]) == int(pair_text_len(c.pairs).sum()) and e["text"].count(b"\n") == len(c.nks)
