"""The frame every per-read device consumer shares, at its edges, in every consumer at once.

A consumer of a step's results is a lane per read: the read's kind decides what the lane loads (kind 1: the record alone; kind 2: nothing; kind 0, and every read
where the step left no records: the pair range from out_offs), then the wave takes its lanes' searched reads one after the other and scans each a row of 64 slots
at a time, most of them with the next row loaded a row ahead.  Hits, cover, depth, segments, read summaries and the screen, classes and the tally, colouring,
pseudoalignment, its paired form, the record gather and the base pileup all repeat that frame; this file pins it where it can go wrong, at the smallest shapes
(the pileup reads the reads themselves, so it takes this case with spelled reads, and ten searched reads more, in tests/test_pileup_records.py):

  - 200 reads: three full waves and one of eight lanes (lanes at and beyond n_reads, a block's last wave);
  - nk cycling through 1, 63, 64, 65, 127, 128, 129, 193: less than a row, exactly one, a second row of one slot, a last row that is empty, full, or one slot;
  - the three kinds interleaved inside a wave, a wave without a searched read, a wave whose only searched reads are lanes 0 and 63;
  - searched reads with a segment that crosses a row boundary upwards and downwards, a row that ends on a found slot while the next begins absent, rows of 2 to 64
    distinct unitigs.
The conditions are asserted on the input itself (assert_frame_conditions), without a GPU.

Three forms: text mode 0 (set_pairs: no records, every read is scanned), text modes 1 and 2 (set_records as tests/test_records_device.py::inject does; in mode 2
the finished reads' pair slots hold GARBAGE).  Every expectation is a host twin's (fa.records_* / fa.expand_records, fin_records_host.cpp) or plain numpy over
one, and every comparison is exact equality."""
from types import SimpleNamespace

import numpy as np
import pytest

import finito_amd as fa
from tests.test_colors_host import assert_pseudo, random_matrix
from tests.test_paired_host import assert_frags
from tests.test_read_class_host import assert_classes, run_labelling, tally_of
from tests.test_read_summary_host import assert_summaries, rule
from tests.test_records import brute_expand
from tests.test_records_device import inject
from tests.test_segments_host import assert_segments
from tests.util import hand_made_case, hand_made_record, random_genome

K = 16
NKS = (1, 63, 64, 65, 127, 128, 129, 193)
N_READS = 200
A = (-1, -1)
_CASE = None


def frame_kinds():
    """the kind of every read.  wave 0: 1, 2, 0 repeating (the searched reads are lanes 2, 5 .. 62); wave 1: no searched read; wave 2: lanes 0 and 63 are the only
    searched reads; the partial wave: all three, searched reads in its first and its last lane"""
    kinds = np.zeros(N_READS, dtype=np.int64)
    kinds[0:64] = (np.arange(64) + 1) % 3
    kinds[64:128] = 1 + (np.arange(64) // 2) % 2
    kinds[128:192] = 1 + np.arange(64) % 2
    kinds[128] = kinds[191] = 0
    kinds[192:200] = (0, 0, 1, 2, 2, 0, 1, 0)
    return kinds


def searched_pairs(j, nk, big):
    """the j-th searched read's nk pairs, by shape j % 5: 0 one ascending run; 1 one descending run; 2 found up to slot 63, absent from slot 64, then another
    unitig downwards; 3 m unitigs taken in turn, m from 2 to 64; 4 absent slots, a run, a repeated pair, an absent end.  big: unitigs of at least 200 k-mers"""
    u, v = int(big[(3 * j) % len(big)]), int(big[(3 * j + 1) % len(big)])
    shape = j % 5
    if shape == 0:
        return [(u, 3 + i) for i in range(nk)]
    if shape == 1:
        return [(u, nk + 1 - i) for i in range(nk)]
    if shape == 2:
        n_abs = min(max(nk - 64, 0), 5)
        return [(u, i) for i in range(min(nk, 64))] + [A] * n_abs + [(v, 199 - i) for i in range(nk - 64 - n_abs)]
    if shape == 3:
        m = (2, 64, 19, 35, 27, 48)[(j // 5) % 6]
        return [(int(big[(j + i % m) % len(big)]), i // m) for i in range(nk)]
    out = [A] * min(3, nk - 1)
    out += [(u, 7 + i) for i in range(max(nk - len(out) - 3, 0))]
    out += [(v, 5)] * min(2, nk - len(out))
    return out + [A] * (nk - len(out))


def frame_case():
    """(made once, nobody changes it) the index of hand_made_case(K), 200 reads whose content is free, hand-made records over them, `pairs` = what they mean"""
    global _CASE
    if _CASE is None:
        c = hand_made_case(K)
        rng = np.random.default_rng(2800)
        kmers = np.diff(np.concatenate([[0], c.ends])) - K + 1
        big = np.nonzero(kmers >= 200)[0]
        assert len(big) >= 64
        nks = np.array([NKS[r % len(NKS)] for r in range(N_READS)], dtype=np.int64)
        kinds = frame_kinds()
        recs = np.zeros(N_READS, dtype=fa.RECORD_DTYPE)
        recs["nk"] = nks
        recs["meta"][kinds == 2] = 2 << 16
        stream = []
        for j, r in enumerate(np.nonzero(kinds == 0)[0]):
            stream += searched_pairs(j, int(nks[r]), big)
        for j, r in enumerate(np.nonzero(kinds == 1)[0]):
            hand_made_record(rng, recs[r:r + 1], int(nks[r]), K, kmers, j % 9, (j // 9) % 2, j % 7)
        stream = np.array(stream, dtype=np.int32).reshape(-1, 2)
        pairs = brute_expand(recs, stream, K)
        all_searched = np.zeros(N_READS, dtype=fa.RECORD_DTYPE)   # the same batch where the step left no records
        all_searched["nk"] = nks
        reads = [random_genome(rng, int(nk) + K - 1) for nk in nks]
        for a in (nks, kinds, recs, stream, pairs, all_searched):
            a.setflags(write=False)
        _CASE = SimpleNamespace(k=K, unitigs=c.unitigs, ends=c.ends, reads=reads, nks=nks, kinds=kinds, recs=recs, stream=stream, pairs=pairs,
                                all_searched=all_searched)
    return _CASE


def assert_frame_conditions(c):
    """what the module's docstring promises of the input, so that an edit of the generator cannot quietly stop producing it"""
    kinds, nks = c.kinds, c.nks
    assert len(nks) == N_READS == 3 * 64 + 8 and np.array_equal(c.recs["meta"] >> 16, kinds)
    for kind in (0, 1, 2):
        assert set(nks[kinds == kind].tolist()) == set(NKS), "kind %d does not meet every nk" % kind
    lanes0 = [np.nonzero(kinds[w:w + 64] == 0)[0].tolist() for w in range(0, N_READS, 64)]
    assert lanes0[0][0] > 0 and lanes0[0][-1] < 63 and len(lanes0[0]) > 10 and all(set(kinds[r:r + 3].tolist()) == {0, 1, 2} for r in range(0, 60))
    assert lanes0[1] == [] and lanes0[2] == [0, 63] and lanes0[3][0] == 0 and lanes0[3][-1] == 7 and set(kinds[192:].tolist()) == {0, 1, 2}
    assert {(int(kinds[2 * f]), int(kinds[2 * f + 1])) for f in range(N_READS // 2)} >= {(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 0), (2, 2)}
    at = np.concatenate([[0], np.cumsum(nks)])
    up = down = found_then_absent = False
    distinct = set()
    for r in np.nonzero(kinds == 0)[0]:
        p = c.pairs[at[r]:at[r + 1]].astype(np.int64)
        for row in range(0, len(p), 64):
            distinct.add(len(np.unique(p[row:row + 64][p[row:row + 64, 0] >= 0, 0])))
        if len(p) > 64:
            same = p[63, 0] >= 0 and p[63, 0] == p[64, 0]
            up |= bool(same and p[64, 1] - p[63, 1] == 1 and p[63, 1] - p[62, 1] == 1)
            down |= bool(same and p[64, 1] - p[63, 1] == -1 and p[63, 1] - p[62, 1] == -1)
            found_then_absent |= bool(p[63, 0] >= 0 and p[64, 0] == -1)
    assert up and down and found_then_absent
    assert {0, 1, 2, 64} <= distinct and any(2 < d < 64 for d in distinct), sorted(distinct)
    assert len(c.pairs) == at[-1] and len(c.stream) == nks[kinds == 0].sum()


def test_the_input_holds_the_edges():
    assert_frame_conditions(frame_case())


def check_every_consumer(p, b, c, recs, stream, what, gathered):
    """the batch holds (recs, stream), the host twins are given the same; gathered: the step left records, so fin_batch_records gathers"""
    k, nks, nu = c.k, c.nks, p.n_unitigs
    pairs, found = fa.expand_records(recs, stream, k)
    assert np.array_equal(pairs, c.pairs)
    want = fa.records_unitig_counts(recs, stream, k, nu)
    h = p.hits()
    try:
        for combine in (0, 4):
            p.set_option("hits_combine", combine)
            counts, total = h.reset().add(b).download()
            assert np.array_equal(counts, want) and total == found, "%s: hits, hits_combine %d" % (what, combine)
    finally:
        p.set_option("hits_combine", None); h.close()
    cv = p.cover()
    bits, covered, total = cv.add(b).download()
    want = fa.records_cover(recs, stream, k, c.ends)
    assert np.array_equal(bits, want) and total == int(covered.sum()) == sum(bin(int(w)).count("1") for w in want), "%s: cover" % what
    cv.close()
    d = p.depth()
    depth, _, total = d.add(b).download()
    assert np.array_equal(depth, fa.records_depth(recs, stream, k, c.ends)) and total == found, "%s: depth" % what
    d.close()
    assert_segments(b.segments(), fa.records_segments(recs, stream, k), "%s: segments" % what)
    summ = fa.records_read_summaries(recs, stream, k)
    assert_summaries(b.read_summaries(), summ, "%s: read summaries" % what)
    for args in ((1, 0, False), (3, 500, True)):
        ids, sbits = b.screen(*args)
        ok = rule(summ, nks, *args)
        assert np.array_equal(ids, np.nonzero(ok)[0]), "%s: screen ids %s" % (what, args)
        assert np.array_equal(np.unpackbits(sbits.view(np.uint8), bitorder="little")[:len(ok)], ok), "%s: screen bits %s" % (what, args)
    rng = np.random.default_rng(2801)
    labels = run_labelling(rng, nu)
    lab = p.labels(labels)
    classes = fa.records_read_classes(recs, stream, k, labels)
    assert_classes(b.classify(lab), classes, "%s: classes" % what)
    for args in ((1, 0, 0), (2, 500, 1)):
        tally, total = lab.reset().add(b, *args).download()
        assert np.array_equal(tally, tally_of(classes, nks, lab.n_labels, *args)) and total == len(nks), "%s: tally %s" % (what, args)
    lab.close()
    for n_colors in (40, 100):   # W = 1 and W = 2
        cbits = random_matrix(rng, nu, n_colors)
        col = p.colors(n_colors, cbits)
        for pm in (0, 500, 1000):
            assert_pseudo(b.pseudoalign(col, pm), fa.records_pseudoalign(recs, stream, k, cbits, n_colors, pm), "%s: %d colours, permille %d" % (what, n_colors, pm))
            for both in (False, True):
                assert_frags(b.pseudoalign_pairs(col, pm, both), fa.records_pseudoalign_pairs(recs, stream, k, cbits, n_colors, pm, both),
                             "%s: fragments, %d colours, permille %d, both %s" % (what, n_colors, pm, both))
        got, n_set = col.reset().add(b, n_colors - 1).download()
        met = np.unique(pairs[pairs[:, 0] >= 0, 0])
        want = np.zeros_like(cbits); want[met, -1] = np.uint64(1) << np.uint64((n_colors - 1) & 63)
        assert np.array_equal(got, want) and n_set == len(met), "%s: colouring, %d colours" % (what, n_colors)
        col.close()
    if gathered:   # last: the gather stamps nk into the searched reads' records
        got_recs, got_stream = b.records()
        assert got_recs.tobytes() == np.ascontiguousarray(recs).tobytes() and np.array_equal(got_stream, stream), "%s: the record gather" % what


@pytest.fixture(scope="module")
def on_device():
    c = frame_case()
    p = fa.FinimizerIndex.build(c.unitigs, c.k).to_device(0)
    assert np.array_equal(p.export(fa.X_ENDS), c.ends)
    yield c, p
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_the_frame_in_every_consumer(mode, on_device):
    c, p = on_device
    assert_frame_conditions(c)
    b = p.batch(c.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(c.pairs)
    if mode == 0:
        b.set_pairs(c.pairs)
        check_every_consumer(p, b, c, c.all_searched, c.pairs, "text mode 0", False)
    else:
        inject(b, c.recs, c.pairs, mode)
        check_every_consumer(p, b, c, c.recs, c.stream, "text mode %d" % mode, True)
    b.close()
