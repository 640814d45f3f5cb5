"""Record-derived text, segments, read summaries and the record gather at every digit count and boundary (fin_text.hip, fin_segments.hip, fin_readsum.hip).

test_text_and_segments_at_every_digit_count injects the enumerated digit case (tests/util.py::digit_case; its conditions: tests/test_record_digits_host.py)
into a small batch: unitig numbers of 1 to 10 digits, offsets against every power of ten, every kind of multiple of 1000 and 2^31, groups of 128 pairs of 24
bytes at every byte offset modulo 16 -- on the searched reads' path of the record text as well as on the finished reads'.  The reference is
tests/test_records.py::brute_expand with plain Python formatting, the segment definition of tests/test_segments_host.py and the summaries' definition of
tests/test_read_summary_host.py.  Hits, bitmap, depth, classes and colour rows index by unitig and are not run on this batch (places outside the index:
tests/test_records_device.py).

test_real_run_with_five_digit_unitigs_and_six_digit_offsets gives the same consumers the PRODUCER's records where the suite's other indexes never are: more
than 12 000 unitigs and one of more than 120 000 bases, against the oracle's pairs.  Every comparison is exact equality."""
import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.test_read_summary_host import assert_summaries, summaries_of
from tests.test_record_digits_host import assert_text, expected, ndigits, text_of
from tests.test_records_device import inject
from tests.test_segments_host import assert_segments, segments_of
from tests.util import cut_unitigs, digit_case, mosaic_read, random_genome, rc, sample_reads

pytestmark = pytest.mark.gpu

FAST_DONE = 4 * 8 + 9   # fin_batch_pipeline_counts word: reads finished by the fast path


def check_record_consumers(b, want, mode, what, pairs, recs=None, stream=None, k=None):
    """text, the count taken from the text pass, pairs, segments, summaries, the gather: `want` = {text, found, segments, summaries} of `pairs`.  With recs and
    stream the gather must return them; without, what it returns must expand to the pairs"""
    assert_text(b.text(), want["text"], what)
    assert b.download(want_pairs=False)[1] == want["found"], "%s: the count taken from the text pass" % what
    if mode == 2:
        with pytest.raises(fa.FinitoError):   # a text-only batch: its pairs stay refused
            b.download()
    else:
        got = b.download()[0]
        bad = np.nonzero((got != pairs).any(axis=1))[0]
        assert len(bad) == 0, "%s: %d pairs differ, first %d: got %s, want %s" % (what, len(bad), bad[0], got[bad[0]], pairs[bad[0]])
    assert_segments(b.segments(), want["segments"], "%s: segments" % what)
    assert_summaries(b.read_summaries(), want["summaries"], "%s: summaries" % what)
    got_recs, got_stream = b.records()
    if recs is not None:
        assert got_recs.tobytes() == np.ascontiguousarray(recs).tobytes(), "%s: records (first differing read %s)" % (what, np.nonzero(got_recs != recs)[0][:1])
        assert np.array_equal(got_stream, stream), "%s: stream" % what
    else:
        assert np.array_equal(fa.expand_records(got_recs, got_stream, k)[0], pairs), "%s: the gathered records do not expand to the pairs" % what
    assert_text(b.text(), want["text"], "%s, the text once more after the other consumers" % what)


@pytest.fixture(scope="module")
def digit_index():
    c = digit_case()
    p = fa.FinimizerIndex.build(c.unitigs, c.k).to_device(0)
    assert np.array_equal(p.export(fa.X_ENDS), c.ends)
    yield p
    p.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_text_and_segments_at_every_digit_count(mode, digit_index):
    c, want = digit_case(), expected()
    b = digit_index.batch(c.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(c.pairs)
    inject(b, c.recs, c.pairs, mode)
    check_record_consumers(b, want, mode, "digit case, text mode %d" % mode, c.pairs, c.recs, c.stream)
    b.close()


def crossings(pairs, lo):
    """how often two neighbouring slots of one unitig hold offsets (lo, lo + 1) and (lo + 1, lo): a read along the unitig, and one against it"""
    same = (pairs[1:, 0] == pairs[:-1, 0]) & (pairs[1:, 0] >= 0)
    up = same & (pairs[:-1, 1] == lo) & (pairs[1:, 1] == lo + 1)
    down = same & (pairs[:-1, 1] == lo + 1) & (pairs[1:, 1] == lo)
    return int(up.sum()), int(down.sum())


def test_real_run_with_five_digit_unitigs_and_six_digit_offsets():
    """a real search: unitig numbers of 4 and 5 digits in the fast path's own records (the short unitigs themselves as reads), offsets of 5 and 6 digits along a
    unitig of 125 000 bases on both strands, reads of several unitigs, mosaics, two reads of more than 4 096 k-mers -- text modes 0, 1 and 2 and the streaming
    text entry against the oracle's pairs"""
    k = 31
    rng = np.random.default_rng(31031)
    g_short, g_long = random_genome(rng, 200000), random_genome(rng, 125000)
    short = cut_unitigs(rng, g_short, k, max_len=60)
    unitigs = short + [g_long]
    assert len(short) >= 12000 and len(g_long) >= 120000
    p, o = fa.FinimizerIndex.build(unitigs, k).to_device(0), OracleIndex.build(unitigs, k)
    assert p.n_unitigs == len(unitigs) >= 12001 and int(np.diff(np.concatenate([[0], o.ends()])).max()) == len(g_long)
    reads = sample_reads(rng, g_long, 2000, 150, err=0.01, random_frac=0.05) + sample_reads(rng, g_short, 500, 150, err=0.01, random_frac=0.05)
    for j in rng.permutation(len(short))[:1500]:     # a short unitig is a read the fast path can finish: one unitig, 1 to 30 k-mers
        r = list(short[j])
        if j % 4 == 0:
            w = int(rng.integers(0, len(r))); r[w] = "ACGT"[("ACGT".index(r[w]) + 1) % 4]
        reads.append("".join(r) if j % 2 else rc("".join(r)))
    for at in (10000, 100000):                       # reads of the fast path's length across the offsets' fifth and sixth digit, along the unitig and against it
        for d in (20, 75, 130, 149 - k, 1):
            reads += [g_long[at - d:at - d + 150], rc(g_long[at - d:at - d + 150])]
    reads += [mosaic_read(rng, g_long + g_short, k, 400) for _ in range(300)]
    reads += [g_long[7000:7000 + 4200 + k], rc(g_long[97000:97000 + 5000 + k])]
    reads = [r for r in reads if len(r) >= k]       # (the text formatter wants a k-mer in every read)
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    nks = np.array([len(r) - k + 1 for r in reads], dtype=np.int64)
    assert (nks > 4096).sum() == 2
    exp = o.search_batch(reads, n_threads=8)[0]
    # conditions on the oracle's pairs
    fnd = exp[exp[:, 0] >= 0]
    digits_u = np.array([ndigits(u) for u in np.unique(fnd[:, 0])])
    assert (digits_u == 4).sum() >= 1000 and (digits_u == 5).sum() >= 1000, np.bincount(digits_u)
    for lo in (9999, 99999):
        up, down = crossings(exp, lo)
        assert up >= 3 and down >= 3, "offsets %d / %d: %d reads along the unitig, %d against it" % (lo, lo + 1, up, down)
    assert fnd[:, 1].max() >= 120000
    pairs = exp.astype(np.int32)
    want = dict(text=text_of(exp, nks), found=len(fnd), segments=segments_of(exp, nks), summaries=summaries_of(exp, nks))
    for mode in (0, 1, 2):
        what = "real run, text mode %d" % mode
        b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        assert b.pipeline_counts(48)[FAST_DONE] > 0.4 * len(reads), "%s: the fast path finished %d of %d reads" % (what, b.pipeline_counts(48)[FAST_DONE], len(reads))
        if mode:   # the producer's records: unitig numbers of 4 and 5 digits, first offsets of 5 and 6, both strands
            recs, _ = b.records()
            one = recs[recs["meta"] >> 16 == 1]
            for s in (0, 1):
                strand = one[(one["meta"] >> 8) & 1 == s]
                assert {4, 5} <= {ndigits(u) for u in strand["u"]} and {5, 6} <= {ndigits(x) for x in strand["off0"]}, "%s, strand %d" % (what, s)
        check_record_consumers(b, want, mode, what, pairs, k=k)
        b.close()
    p.set_option("pipeline_kmers", 30000)            # sub-batches in text mode 2, several in flight
    try:
        got, npos = p.search_reads_text(reads)
    finally:
        p.set_option("pipeline_kmers", None)
    assert_text(got, want["text"], "the streaming text entry")
    assert npos == want["found"]
    p.close()
