"""Every device consumer of fast-path records on HAND-MADE records (fin_batch_set_records; tests/util.py::hand_made_records).

The pair pre-pass writes records with at most four positions, for reads of at most 256 bases, and a search's own output is all the device consumers had ever seen:
the record-derived text (fin_text.hip), fin_hits_rec_kernel, fin_cover_rec_kernel, fin_depth_rec_kernel, the kind-1 branch of fin_sgm_kernel and the gather of
fin_batch_records.  Here they are given the whole format: five to eight positions (the second position word), gaps that touch, overlap, coincide, are clamped at
slot 0 or at nk - 1, cover every slot; reads of thousands of k-mers over several text segments and more than 64 bitmap words; places outside the index.

The reference is always tests/test_records.py::brute_expand -- the record's meaning in three lines -- over the hand-made records and the hand-made pairs of the
searched reads; each consumer's expectation is plain numpy over those pairs (np.bincount, np.unique, the segment definition of tests/test_segments_host.py,
oracle.oracle.format_pairs).  Nothing is expected from fin_expand_records, fin_records_* or a device output, and every comparison is exact equality.

The base pileup (fin_pileup_add_kernel's kind-1 branch) is a consumer of the same records, but it trusts them where its definition reads the text: it needs reads
spelled to agree with their records and faces these cases, through `inject`, in tests/test_pileup_records.py.

Out of reach from here: the pre-pass's own pair writer for a finished read (fin_prepass.hip; its branch for more than four positions).  It is the producer, not a
consumer: hand-made records do not pass through it, and it cannot run while FIN_FAST_MAXE is 4."""
import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import OracleIndex, format_pairs
from tests import test_unitig_coverage as cov
from tests import test_unitig_depth as dep
from tests.test_records import brute_expand
from tests.test_records_host import assert_generator_conditions, positions_of
from tests.test_segments_host import assert_segments, segments_of
from tests.test_unitig_counts import profile_of
from tests.util import cut_unitigs, hand_made_case, hand_made_record, random_genome, sample_reads, searched_read_pairs

GARBAGE = (0x7FFFFFF0, 7)   # what a finished read's pair slots hold in text mode 2: no record consumer may read them


@pytest.fixture(scope="module")
def on_device():
    made = {}

    def get(k):
        if k not in made:
            c = hand_made_case(k)
            made[k] = fa.FinimizerIndex.build(c.unitigs, k).to_device(0)
            assert np.array_equal(made[k].export(fa.X_ENDS), c.ends)
        return made[k]
    yield get
    for p in made.values():
        p.close()


def device_form(recs):
    """as the step leaves them: a searched read's record is all zero (fin_batch_records stamps nk later)"""
    out = np.array(recs)
    out[out["meta"] >> 16 == 0] = np.zeros(1, dtype=fa.RECORD_DTYPE)[0]
    return out


def inject(b, recs, pairs, mode):
    """the records over the run's, and the pairs: in text mode 1 every read's, in mode 2 garbage where a finished read's pairs would be"""
    slots = np.array(pairs, dtype=np.int32)
    if mode == 2:
        slots[np.repeat(recs["meta"] >> 16 != 0, recs["nk"])] = GARBAGE
    b.set_records(device_form(recs), slots)


def text_of(pairs, nks):
    at = np.concatenate([[0], np.cumsum(nks)])
    return "".join(format_pairs(pairs[at[r]:at[r + 1]]) for r in range(len(nks))).encode()


def check_every_consumer(p, b, recs, stream, pairs, ends, mode, what):
    """the batch holds (recs, stream); pairs = brute_expand of them"""
    nks = recs["nk"].astype(np.int64)
    found = int((pairs[:, 0] != -1).sum())
    want_profile = profile_of(pairs, p.n_unitigs)
    h = p.hits()
    try:
        for combine in (0, 1, 4):
            p.set_option("hits_combine", combine)
            counts, total = h.reset().add(b).download()
            assert np.array_equal(counts, want_profile) and total == found, "%s: profile, hits_combine %d" % (what, combine)
            counts, total = h.add(b).download()
            assert np.array_equal(counts, 2 * want_profile) and total == 2 * found, "%s: profile added twice, hits_combine %d" % (what, combine)
    finally:
        p.set_option("hits_combine", None); h.close()
    want_cover = cov.Want(pairs, ends)
    c = p.cover()
    try:
        for probe in (0, 1):
            p.set_option("cover_probe", probe)
            cov.assert_cover(c.reset().add(b).download(), want_cover, "%s: bitmap, cover_probe %d" % (what, probe))
            cov.assert_cover(c.add(b).download(), want_cover, "%s: bitmap added twice, cover_probe %d" % (what, probe))
    finally:
        p.set_option("cover_probe", None); c.close()
    want_depth = dep.Want(pairs, ends)
    d = p.depth()
    dep.assert_depth(d.add(b).download(min_depth=2), want_depth, "%s: depth" % what, min_depth=2)
    dep.assert_depth(d.add(b).download(), want_depth.times(2), "%s: depth added twice" % what)
    d.close()
    assert_segments(b.segments(), segments_of(pairs, nks), "%s: segments" % what)
    got_text, want_text = b.text(), text_of(pairs, nks)
    if got_text != want_text:
        i = next((j for j, (x, y) in enumerate(zip(got_text, want_text)) if x != y), min(len(got_text), len(want_text)))
        raise AssertionError("%s: text of %d bytes, expected %d; first difference at byte %d (line %d): got %r, want %r" %
                             (what, len(got_text), len(want_text), i, want_text[:i].count(b"\n"), got_text[max(0, i - 30):i + 30], want_text[max(0, i - 30):i + 30]))
    assert b.download(want_pairs=False)[1] == found, "%s: the count taken from the text pass" % what
    if mode == 2:
        with pytest.raises(fa.FinitoError):   # still a text-only batch: its pairs stay refused
            b.download()
    else:
        assert np.array_equal(b.download()[0], pairs)
    got_recs, got_stream = b.records()
    assert got_recs.tobytes() == np.ascontiguousarray(recs).tobytes(), "%s: records (first differing read %s)" % (what, np.nonzero(got_recs != recs)[0][:1])
    assert np.array_equal(got_stream, stream), "%s: stream" % what


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("k", [16, 31, 63])
def test_every_consumer_on_hand_made_records(k, mode, on_device):
    c, p = hand_made_case(k), on_device(k)
    b = p.batch(c.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(c.pairs)
    inject(b, c.recs, c.pairs, mode)
    check_every_consumer(p, b, c.recs, c.stream, c.pairs, c.ends, mode, "k=%d text mode %d" % (k, mode))
    b.close()


def long_reads_case():
    """the input of test_long_finished_reads: (k, unitigs, ends, reads, recs, stream, pairs)"""
    k = 31
    rng = np.random.default_rng(4096)
    g = random_genome(rng, 40000)
    unitigs = [g[0:12000], g[12000 - (k - 1):24000], g[24000 - (k - 1):36000]] + cut_unitigs(rng, g[36000 - (k - 1):], k, max_len=700)
    ends = OracleIndex.build(unitigs, k).ends()
    kmers = np.diff(np.concatenate([[0], ends])) - k + 1
    long_lens = [300, 1000, 4095 + k, 4096 + k, 4097 + k, 9000 + k]
    lens, forced = [], {}
    for j, L in enumerate(long_lens + long_lens):
        lens += [int(x) for x in rng.integers(k, 301, int(rng.integers(5, 40)))]
        forced[len(lens)] = ((0, 5, 8)[(j + j // 6) % 3], j // 6)   # read number -> (positions, strand)
        lens.append(L)
    lens += [int(x) for x in rng.integers(k, 301, 30)]
    nks = np.array(lens) - k + 1
    recs = np.zeros(len(lens), dtype=fa.RECORD_DTYPE)
    recs["nk"] = nks
    stream = []
    for r, nk in enumerate(nks):
        kind = 1 if r in forced else int(rng.integers(0, 3))
        if kind == 0:
            stream += searched_read_pairs(rng, int(nk), kmers)
        elif kind == 2:
            recs["meta"][r] = 2 << 16
        else:
            nE, rev = forced.get(r, (int(rng.integers(0, 9)), int(rng.integers(0, 2))))
            hand_made_record(rng, recs[r:r + 1], int(nk), k, kmers, nE, rev, 0 if r in forced else int(rng.integers(0, 7)))
    stream = np.array(stream, dtype=np.int32).reshape(-1, 2)
    pairs = brute_expand(recs, stream, k)
    # conditions on the inputs: the long reads keep found stretches beyond the first text segment and cross more than 64 bitmap words
    at = np.concatenate([[0], np.cumsum(nks)])
    for r in forced:
        assert (pairs[at[r] + int(nks[r]) // 2:at[r + 1], 0] != -1).any() and (pairs[at[r]:at[r + 1], 0] != -1).sum() > 100
    assert sum(int(nks[r]) > 64 * 64 for r in forced) >= 6 and {int(recs["meta"][r]) & 0xFF for r in forced} == {0, 5, 8}
    reads = [random_genome(rng, L) for L in lens]
    return k, unitigs, ends, reads, recs, stream, pairs


@pytest.mark.gpu
def test_long_finished_reads():
    """kind-1 reads of 270 to 9 001 k-mers -- around FIN_TEXT_SEG = 4 096 pairs, where the text formatter cuts a read into segments, and over more than 64 words
    of the bitmap -- on either strand with 0, 5 and 8 positions, between short reads of every kind"""
    k, unitigs, ends, reads, recs, stream, pairs = long_reads_case()
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    assert np.array_equal(p.export(fa.X_ENDS), ends)
    for mode in (1, 2):
        b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        inject(b, recs, pairs, mode)
        check_every_consumer(p, b, recs, stream, pairs, ends, mode, "long reads, text mode %d" % mode)
        b.close()
    p.close()


@pytest.mark.parametrize("k", [16, 31, 63])
def test_the_pre_pass_shapes_alone_are_not_enough(k):
    """a guard on the generator, not on the device: the records of test_every_consumer_on_hand_made_records hold what the conditions of
    tests/test_records_host.py ask for, and most of them are records the pre-pass cannot write today (more than four positions)"""
    c = hand_made_case(k)
    assert_generator_conditions(c)
    one = c.recs["meta"] >> 16 == 1
    beyond = one & ((c.recs["meta"] & 0xFF) > 4)
    assert beyond.sum() >= 800 and (c.recs["Es2"][beyond] != 0).sum() >= 700
    assert all(positions_of(r) == sorted(positions_of(r)) for r in c.recs[one])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_set_records_then_a_real_run(mode, on_device):
    """nothing of an injection survives a reload and a run: text, profile, segments and pairs of real reads on the same batch are the oracle's"""
    k = 31
    c, p = hand_made_case(k), on_device(k)
    o = OracleIndex.build(c.unitigs, k)
    b = p.batch(c.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
    inject(b, c.recs, c.pairs, mode)
    b.segments(); b.text(); b.records()   # everything the batch may remember of the injected records
    rng = np.random.default_rng(12)
    reads = sample_reads(rng, c.genome, 700, 150, err=0.01, random_frac=0.05) + sample_reads(rng, c.genome, 100, 290, err=0.03)
    exp = o.search_batch(reads, n_threads=8)[0]
    nks = np.array([len(r) - k + 1 for r in reads])
    b.reload(reads); b.run(fa.FIN_MERGED)
    got_recs, got_stream = b.records()
    assert (got_recs["meta"] >> 16 == 1).sum() > 100, "the real run's fast path finished reads"
    assert np.array_equal(fa.expand_records(got_recs, got_stream, k)[0].astype(np.int64), exp)
    assert b.text() == text_of(exp, nks)
    h = p.hits()
    counts, total = h.add(b).download()
    assert np.array_equal(counts, profile_of(exp, p.n_unitigs)) and total == int((exp[:, 0] != -1).sum()) == b.download(want_pairs=False)[1]
    h.close()
    assert_segments(b.segments(), segments_of(exp, nks), "segments of the real run")
    if mode == 1:
        assert np.array_equal(b.download()[0].astype(np.int64), exp)
    b.close()


@pytest.mark.gpu
def test_set_records_refuses_what_the_kernels_would_trust(on_device):
    """the host-side checks of fin_batch_set_records: nothing is copied when one fails, and a run that left no records has none to overwrite"""
    k = 31
    c, p = hand_made_case(k), on_device(k)
    b = p.batch(c.reads)
    good = device_form(c.recs)
    with pytest.raises(fa.FinitoError) as e:   # no run yet
        b.set_records(good)
    assert e.value.code == fa.FIN_EINVAL
    b.text_mode(0); b.run(fa.FIN_MERGED)
    with pytest.raises(fa.FinitoError) as e:   # text mode 0 leaves no records
        b.set_records(good)
    assert e.value.code == fa.FIN_EINVAL and "no records" in str(e.value)
    b.text_mode(2); b.run(fa.FIN_MERGED)
    ran = profile_of(OracleIndex.build(c.unitigs, k).search_batch(c.reads, n_threads=8)[0], p.n_unitigs)   # what the run itself found
    one = int(np.nonzero((c.recs["meta"] >> 16 == 1) & ((c.recs["meta"] & 0xFF) == 3) & (c.recs["nk"] > 5))[0][0])
    two = int(np.nonzero(c.recs["meta"] >> 16 == 2)[0][0])
    zero = int(np.nonzero(c.recs["meta"] >> 16 == 0)[0][0])
    nk = int(c.recs["nk"][one])

    def kind3(r): r["meta"][one] = (3 << 16) | 3
    def nk_short(r): r["nk"][one] = nk - 1
    def nk_long(r): r["nk"][two] += 1
    def nk_none(r): r["nk"][two] = 0
    def nine(r): r["meta"][one] = (1 << 16) | 9
    def descend(r): r["Es"][one] = 7 | (6 << 16) | (9 << 32)
    def beyond(r): r["Es"][one] = 1 | (2 << 16) | ((nk + k - 1) << 32)
    def unused(r): r["Es2"][one] = 5
    def unused_low(r): r["Es"][one] = 1 | (2 << 16) | (3 << 32) | (4 << 48)
    def stamped(r): r["nk"][zero] = c.recs["nk"][zero]
    def placed(r): r["u"][zero] = 1
    for change in (kind3, nk_short, nk_long, nk_none, nine, descend, beyond, unused, unused_low, stamped, placed):
        bad = good.copy(); change(bad)
        with pytest.raises(fa.FinitoError) as e:
            b.set_records(bad, np.zeros((b.n_kmers, 2), np.int32))
        assert e.value.code == fa.FIN_EINVAL and "record %d" % {nk_long: two, nk_none: two, stamped: zero, placed: zero}.get(change, one) in str(e.value), change.__name__
    with pytest.raises(fa.FinitoError):        # a record too few
        b.set_records(good[:-1])
    h = p.hits()
    assert np.array_equal(h.add(b).download()[0], ran), "a refused call copied something"
    edge = good.copy(); edge["Es"][one] = 1 | (2 << 16) | ((nk + k - 2) << 32)   # the highest position the format has is legal
    slots = np.array(c.pairs); slots[np.repeat(c.recs["meta"] >> 16 != 0, c.recs["nk"])] = GARBAGE
    b.set_records(edge, slots)
    logical = np.array(c.recs); logical["Es"][one] = edge["Es"][one]
    counts, _ = h.reset().add(b).download()
    assert np.array_equal(counts, profile_of(brute_expand(logical, c.stream, k), p.n_unitigs))
    h.close(); b.close()


@pytest.mark.gpu
def test_record_places_outside_the_index(on_device):
    """four kind-1 records whose place is no place of the index -- a unitig number just beyond the set, a record that runs off the text by ten slots, one that lies
    wholly beyond it, unitig 0xFFFFFFFE -- among the good ones: hits, bitmap and depth skip exactly what lies outside, count everything else and say FIN_EINVAL
    "outside the index" until the reset.  (Segments and text have no notion of the index and are not run on this set.)"""
    k = 31
    c, p = hand_made_case(k), on_device(k)
    n_unitigs, total_len = p.n_unitigs, p.total_len
    starts = np.concatenate([[0], c.ends[:-1]])
    last_len = int(c.ends[-1] - starts[-1])
    at = np.concatenate([[0], np.cumsum(c.nks)])
    one = (c.recs["meta"] >> 16 == 1) & ((c.recs["meta"] & 0xFF) <= 2) & (c.recs["nk"] >= 40)
    one[768:1024] = False
    off_text = int(np.nonzero(one & (c.recs["nk"] <= last_len + 10))[0][0])   # room for off0 >= 0 in the last unitig
    others = [int(r) for r in np.nonzero(one)[0] if r != off_text][:3]
    recs = np.array(c.recs)
    recs["u"][others[0]] = n_unitigs + 5
    recs["u"][off_text], recs["off0"][off_text] = n_unitigs - 1, last_len - int(c.recs["nk"][off_text]) + 10
    recs["u"][others[1]], recs["off0"][others[1]] = n_unitigs - 1, last_len + 1000
    recs["u"][others[2]] = 0xFFFFFFFE
    # the expectation: the two records of no unitig mean nothing; the other two mean what brute_expand says, and a place at or beyond the text's end is no place
    pairs = np.array(c.pairs)
    for r in (others[0], others[2]):
        pairs[at[r]:at[r + 1]] = -1
    for r in (off_text, others[1]):
        pairs[at[r]:at[r + 1]] = brute_expand(recs[r:r + 1], np.zeros((0, 2), np.int32), k)
    want_profile = profile_of(pairs, n_unitigs)                                     # (a profile knows unitigs, not places)
    inside = pairs.copy()
    fnd = inside[:, 0] >= 0
    beyond = np.zeros(len(inside), dtype=bool)
    beyond[fnd] = starts[inside[fnd, 0]] + inside[fnd, 1] >= total_len
    assert 10 <= beyond[at[off_text]:at[off_text + 1]].sum() < (pairs[at[off_text]:at[off_text + 1], 0] >= 0).sum() and beyond[at[others[1]]:at[others[1] + 1]].all()
    inside[beyond] = -1
    want_cover, want_depth = cov.Want(inside, c.ends), dep.Want(inside, c.ends)
    good_cover, good_depth = cov.Want(c.pairs, c.ends), dep.Want(c.pairs, c.ends)
    assert want_depth.found < good_depth.found

    b = p.batch(c.reads); b.text_mode(2); b.run(fa.FIN_MERGED)
    h, cv, d = p.hits(), p.cover(), p.depth()
    inject(b, recs, pairs, 2)
    for acc in (h, cv, d):
        acc.add(b)
        for _ in range(2):   # ... until the reset
            with pytest.raises(fa.FinitoError) as e:
                acc.download()
            assert e.value.code == fa.FIN_EINVAL and "outside the index" in str(e.value)
    # everything else was counted: the accumulators themselves, read through their device pointers
    counts = dep.device_int32(h.device_ptr(), 2 * n_unitigs).view(np.uint64)
    assert np.array_equal(counts, want_profile)
    bits = dep.device_int32(cv.device_ptr(), 2 * len(want_cover.bits)).view(np.uint64)
    assert np.array_equal(bits, want_cover.bits)
    diff = dep.device_int32(d.device_ptr(), total_len + 1)
    assert int(diff.astype(np.int64).sum()) == 0 and np.array_equal(np.cumsum(diff[:-1].astype(np.int64)), want_depth.depth), "half a range was written"
    # after the reset the good set alone is exact
    inject(b, c.recs, c.pairs, 2)
    counts, total = h.reset().add(b).download()
    assert np.array_equal(counts, profile_of(c.pairs, n_unitigs)) and total == good_depth.found
    cov.assert_cover(cv.reset().add(b).download(), good_cover, "after the reset")
    dep.assert_depth(d.reset().add(b).download(), good_depth, "after the reset")
    h.close(); cv.close(); d.close(); b.close()
