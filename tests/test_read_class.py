"""Read classification by unitig labels, on the device (include/finito_amd.h: fin_labels_*, fin_batch_classify, fin_batch_add_classes, fin_search_batch_classify,
fin_search_batch_add_classes, fin_index_unitig_numbers; fin_classify.hip).  The expectation is always the definition written in numpy
(tests/test_read_class_host.py::classes_of, ::assigned) over the ORACLE's pairs -- or, for hand-made records and hand-made pairs, over those pairs -- never a device
output or a fin_records_* result; every comparison is exact."""
import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.test_read_class_host import NONE, assert_classes, classes_of, run_labelling, tally_of
from tests.test_read_summary_host import assert_summaries, summaries_of
from tests.test_records_device import inject
from tests.test_segments import nks_of, oracle_pairs
from tests.test_segments_host import assert_segments, segments_of
from tests.test_unitig_counts import read_families
from tests.util import cut_unitigs, hand_made_case, random_genome

pytestmark = pytest.mark.gpu

RULES = [(1, 0, 0), (1, 0, 1), (10, 500, 0), (0, 1000, 0), (3, 200, 2)]   # (min_found, min_permille, min_margin)


def numbers_of(unitigs, k):
    """the index's number of every input unitig, finito_amd.synth.unitig_ids' rule restated: the rank of its reversed first k-mer, ties by input order"""
    order = np.argsort(np.array([u[:k][::-1] for u in unitigs]), kind="stable")
    out = np.empty(len(unitigs), dtype=np.int64)
    out[order] = np.arange(len(unitigs))
    return out


def hand_picked_reads(unitigs, k, labels):
    """reads whose classes show what a random draw may lack: a tie, found k-mers that are all unlabelled, labelled and unlabelled ones in one read"""
    lab = labels[numbers_of(unitigs, k)]   # in input order
    named = [i for i in range(len(unitigs)) if lab[i] != NONE]
    bare = [i for i in range(len(unitigs)) if lab[i] == NONE]
    a = named[0]
    b = next(i for i in named if lab[i] != lab[a])
    m = min(len(unitigs[a]), len(unitigs[b]), len(unitigs[bare[0]]))
    return [unitigs[a][:m] + unitigs[b][:m], unitigs[b][:m] + unitigs[a][:m], unitigs[bare[0]], unitigs[a][:m] + unitigs[bare[0]][:m]]


def assert_expectation_shows_everything(want, pairs, nks):
    found = np.array([int((pairs[a:b, 0] != -1).sum()) for a, b in zip(np.cumsum(nks) - nks, np.cumsum(nks))])
    assert (want["n_second"] > 0).any(), "no read with a second label"
    assert ((want["n_best"] == want["n_second"]) & (want["n_best"] > 0)).any(), "no tie"
    assert ((found > 0) & (want["n_labelled"] == 0)).any(), "no read whose found k-mers are all unlabelled"
    assert ((want["n_labelled"] > 0) & (want["n_labelled"] < found)).any(), "no read with labelled and unlabelled found k-mers"
    assert ((want["label"] == NONE) & (nks > 0)).any(), "no empty class on a read with k-mers"


@pytest.fixture(scope="module")
def set31():
    rng = np.random.default_rng(21600)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, 31, max_len=700)
    p = fa.FinimizerIndex.build(unitigs, 31).to_device(0)
    o = OracleIndex.build(unitigs, 31)
    labels = run_labelling(rng, len(unitigs))
    reads = read_families(rng, g, 31, unitigs) + hand_picked_reads(unitigs, 31, labels)
    nks = nks_of(reads, 31)
    pairs = oracle_pairs(o, reads)
    want = classes_of(pairs, nks, labels)
    for a in (labels, nks, pairs, want):
        a.setflags(write=False)
    yield p, o, unitigs, labels, reads, nks, want
    p.close()


@pytest.mark.parametrize("k", [16, 31, 63, 127])
def test_classes_of_every_read_family_in_every_text_mode(k):
    """text modes 0, 1 and 2: in modes 1 and 2 the fast path's reads are classified from their records (in mode 2 their pairs do not exist); k = 127 leaves no
    records, every read goes through the pair scan.  The call changes neither records nor pairs nor text nor segments nor summaries"""
    rng = np.random.default_rng(1600 + k)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=max(700, 4 * k))
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    labels = run_labelling(rng, len(unitigs))
    other = np.roll(labels, len(labels) // 3)
    reads = read_families(rng, g, k, unitigs) + hand_picked_reads(unitigs, k, labels)
    nks = nks_of(reads, k)
    e1 = oracle_pairs(o, reads)
    want, want_other = classes_of(e1, nks, labels), classes_of(e1, nks, other)
    assert_expectation_shows_everything(want, e1, nks)
    assert not np.array_equal(want, want_other)
    want_segs, want_sums = segments_of(e1, nks), summaries_of(e1, nks)
    found = int((e1[:, 0] != -1).sum())
    full = [r for r in reads if len(r) >= k]
    want_full = classes_of(oracle_pairs(o, full), nks_of(full, k), labels)
    lab, lab2 = p.labels(labels), p.labels(other)
    assert lab.n_labels == 7 and all(lab.device_ptrs())
    for mode in (0, 1, 2):
        b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        assert b.device_read_classes_ptr() == 0
        got = b.classify(lab)
        assert_classes(got, want, "k=%d text mode %d" % (k, mode))
        assert b.device_read_classes_ptr() != 0
        info = b.run_info()
        if k <= 63:
            assert info["fast_path"] and (mode == 0 or b.pipeline_counts()[41] > 0)   # the record path was really taken (modes 1 and 2)
        else:
            assert not info["fast_path"] and b.pipeline_counts()[41] == 0   # no records: every read goes through the scan
        assert_classes(b.classify(lab), want, "k=%d text mode %d, a second call" % (k, mode))
        assert_classes(b.classify(lab2), want_other, "k=%d text mode %d, another labelling" % (k, mode))
        assert_classes(b.classify(lab), want, "k=%d text mode %d, the first labelling again" % (k, mode))
        # everything else the batch gives is what it gives without the call
        assert_segments(b.segments(), want_segs, "k=%d text mode %d, segments after the classes" % (k, mode))
        assert_summaries(b.read_summaries(), want_sums, "k=%d text mode %d, summaries after the classes" % (k, mode))
        if mode == 2 and info["fast_path"]:
            with pytest.raises(fa.FinitoError):
                b.download()
        else:
            pairs, n = b.download()
            assert n == found and np.array_equal(pairs.astype(np.int64), e1)
        assert_classes(b.classify(lab), want, "k=%d text mode %d, after segments, summaries and download" % (k, mode))
        b.reload(full)
        with pytest.raises(fa.FinitoError) as e:   # reloaded, not run yet
            b.classify(lab)
        assert e.value.code == fa.FIN_EINVAL and b.device_read_classes_ptr() == 0
        b.run(fa.FIN_MERGED)
        assert b.device_read_classes_ptr() == 0
        assert_classes(b.classify(lab), want_full, "k=%d text mode %d, reads with k-mers" % (k, mode))
        b.close()
    lab.close(); lab2.close()
    p.close()


def test_forward_only(set31):
    p, o, unitigs, labels, reads, nks, _ = set31
    want = classes_of(oracle_pairs(o, reads[:500], fa.FIN_FWD), nks[:500], labels)
    assert (want["n_labelled"] > 0).sum() > 100 and not np.array_equal(want, set31[6][:500])
    lab = p.labels(labels)
    for mode in (0, 2):
        b = p.batch(reads[:500]); b.text_mode(mode); b.run(fa.FIN_FWD)
        assert_classes(b.classify(lab), want, "forward only, mode %d" % mode)
        b.close()
    assert_classes(p.classify_reads(reads[:500], lab, fa.FIN_FWD), want, "forward only, host buffers")
    lab.close()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("k", [16, 31, 63])
def test_hand_made_records_on_the_device(k, mode):
    """the whole record format through the kind-1 branch: labelled and unlabelled unitigs, nk = 0 after the gaps (every slot absent), kind 2, both strands (meta bit
    8), all three kinds in every wave; in mode 2 a finished read's pair slots hold garbage, which nobody may read"""
    c = hand_made_case(k)
    rng = np.random.default_rng(1650 + k)
    labels = run_labelling(rng, len(c.unitigs))
    want = classes_of(c.pairs, c.nks, labels)
    kinds, rev = c.recs["meta"] >> 16, (c.recs["meta"] >> 8) & 1
    found = np.add.reduceat((c.pairs[:, 0] != -1).astype(np.int64), np.concatenate([[0], np.cumsum(c.nks)[:-1]]))
    one = kinds == 1
    assert (one & (labels[c.recs["u"]] == NONE) & (found > 0)).any() and (one & (labels[c.recs["u"]] != NONE) & (found > 0) & (rev == 1)).any()
    assert (one & (labels[c.recs["u"]] != NONE) & (found == 0)).any() and (kinds == 2).any() and (want[kinds == 0]["n_second"] > 0).any()
    p = fa.FinimizerIndex.build(c.unitigs, k).to_device(0)
    lab = p.labels(labels)
    b = p.batch(c.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(c.pairs)
    b.classify(lab)
    inject(b, c.recs, c.pairs, mode)
    assert b.device_read_classes_ptr() == 0   # forgotten
    assert_classes(b.classify(lab), want, "k=%d text mode %d" % (k, mode))
    for rule in RULES:
        reads, total = lab.reset().add(b, *rule).download()
        assert np.array_equal(reads, tally_of(want, c.nks, 7, *rule)) and total == len(c.reads), "k=%d text mode %d rule %s" % (k, mode, rule)
    b.close(); lab.close()
    p.close()


@pytest.fixture(scope="module")
def wide():
    """an index of more than 200 unitigs, one label per unitig: a read's distinct labels are the distinct unitigs of its hand-made pairs"""
    k = 31
    rng = np.random.default_rng(1664)
    g = random_genome(rng, 12000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, k, max_len=80), k).to_device(0)
    assert p.n_unitigs >= 200
    yield p, rng
    p.close()


def test_reads_with_more_labels_than_the_table_holds(wide):
    """hand-made pairs (set_pairs, text mode 0: every read is scanned): 64 distinct labels fill the wave's table, 65 and 130 overflow it; the class stays exact"""
    p, rng = wide
    k, nu = 31, p.n_unitigs
    A = (-1, -1)
    cases = {}
    cases["64 labels"] = [(u, 0) for u in range(100, 164) for _ in range(2)] + [(131, 1)]
    cases["65 labels"] = [(u, 0) for u in range(100, 165) for _ in range(2)] + [(164, 1)]
    cases["65 labels, descending"] = [(u, 0) for u in range(164, 99, -1) for _ in range(2)] + [(100, 1)]
    # 130 labels, the winner among the last to appear and numerically among the largest: it is dropped from the first pass and counted in the last
    order = [int(u) for u in rng.permutation(130)]
    order.remove(128); order.insert(127, 128)
    cases["130 labels, a late and large winner"] = [(u, 0) for u in order for _ in range(2)] + [(128, 1), (128, 2), A, (3, 0)]
    # 130 labels, the smallest and the largest tie for the best count, a third one is second to both
    cases["130 labels, a tie of the ends"] = [(129, 0)] * 3 + [(u, 0) for u in order] + [(0, 1)] * 3 + [(129, 1), (0, 2), (64, 1)]
    cases["130 labels, every one once, interleaved with absent slots"] = [x for u in order[::-1] for x in ((u, 5), A)]
    cases["200 labels twice over"] = [(u, 0) for u in range(200)] + [(u, 1) for u in range(199, -1, -1)] + [(77, 2)]
    # a label's run across the boundary between rows of 64 slots, in reads of 63, 64, 65 and 129 slots
    for nk in (63, 64, 65, 129):
        for h in (nk - 2, 62, 63, 64):
            if 0 < h < nk:
                cases["%d slots, a run from slot %d" % (nk, h)] = [(7, i) for i in range(h)] + [(9, i) for i in range(nk - h)]
        cases["%d slots, one label" % nk] = [(5, i) for i in range(nk)]
        cases["%d slots, nothing" % nk] = [A] * nk
        cases["%d slots, the last one only" % nk] = [A] * (nk - 1) + [(11, 0)]
    labels = np.arange(nu, dtype=np.uint32)
    names = list(cases)
    pairs = np.array([x for n in names for x in cases[n]], dtype=np.int32)
    nks = np.array([len(cases[n]) for n in names])
    reads = [random_genome(rng, int(nk) + k - 1) for nk in nks]
    want = classes_of(pairs, nks, labels)
    w = dict(zip(names, (tuple(x) for x in want.tolist())))
    # conditions on the expectation, spelled out
    assert w["64 labels"] == (131, 3, 2, 129) and w["65 labels"] == (164, 3, 2, 131) and w["65 labels, descending"] == (100, 3, 2, 131)
    assert w["130 labels, a late and large winner"] == (128, 4, 3, 263) and w["130 labels, a tie of the ends"] == (0, 5, 5, 139)
    assert w["130 labels, every one once, interleaved with absent slots"] == (0, 1, 1, 130) and w["200 labels twice over"] == (77, 3, 2, 401)
    assert w["65 slots, a run from slot 63"] == (7, 63, 2, 65) and w["129 slots, a run from slot 64"] == (9, 65, 64, 129) and w["64 slots, a run from slot 62"] == (7, 62, 2, 64)
    b = p.batch(reads); b.text_mode(0); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(pairs)
    lab = p.labels(labels)
    b.classify(lab)
    b.set_pairs(pairs)
    assert b.device_read_classes_ptr() == 0   # forgotten
    got = b.classify(lab)
    for i, n in enumerate(names):
        assert tuple(got[i].tolist()) == w[n], "%s: got %s, want %s" % (n, got[i], w[n])
    # the same reads under labellings that merge unitigs: few labels (the common case), and exactly 64 and 65 of them over all 200 unitigs
    for n_lab in (3, 64, 65):
        merged = (np.arange(nu) % n_lab).astype(np.uint32)
        merged[::17] = NONE
        lab2 = p.labels(merged, n_lab)
        assert_classes(b.classify(lab2), classes_of(pairs, nks, merged), "hand-made pairs, %d labels" % n_lab)
        reads2, total = lab2.add(b, 1, 0, 1).download()
        assert np.array_equal(reads2, tally_of(classes_of(pairs, nks, merged), nks, n_lab, 1, 0, 1)) and total == len(names)
        lab2.close()
    b.close(); lab.close()


def test_edge_batches_and_refusals(set31):
    p, o, unitigs, labels, reads, nks, want = set31
    rng = np.random.default_rng(1666)
    lab = p.labels(labels)
    nowhere = [random_genome(rng, 200) for _ in range(300)] + ["N" * 200]
    for rd in ([], ["", "AC"], nowhere):
        for mode in (0, 2):
            b = p.batch(rd); b.text_mode(mode); b.run(fa.FIN_MERGED)
            got = b.classify(lab)
            assert len(got) == len(rd) and got.dtype == fa.READ_CLASS_DTYPE
            assert_classes(got, classes_of(oracle_pairs(o, rd), nks_of(rd, 31), labels) if rd else np.zeros(0, fa.READ_CLASS_DTYPE), "%d reads, mode %d" % (len(rd), mode))
            assert (got["label"] == NONE).all() and not got["n_best"].any()
            tally, total = lab.reset().add(b).download()
            assert tally[:-1].sum() == 0 and tally[-1] == total == len(rd)
            b.close()
    b = p.batch(reads[:300]); b.text_mode(2); b.run(fa.FIN_MERGED)
    pairs300 = oracle_pairs(o, reads[:300])
    # a labelling without a label; a labelling of one label
    for lb, n_lab in ((np.full(len(labels), NONE, dtype=np.uint32), None), (np.zeros(len(labels), dtype=np.uint32), None), (np.where(labels == NONE, NONE, 0).astype(np.uint32), 1)):
        l2 = p.labels(lb, n_lab)
        assert l2.n_labels == 1
        w2 = classes_of(pairs300, nks[:300], lb)
        assert_classes(b.classify(l2), w2, "labels %s" % np.unique(lb))
        assert not w2["n_second"].any()
        tally, total = l2.add(b).download()
        assert np.array_equal(tally, tally_of(w2, nks[:300], 1, 1, 0, 0)) and total == 300
        l2.close()
    # what fin_labels_create refuses
    for lb, n_lab in ((labels, 0), (labels, 6), (labels, 0x80000001), (labels[:-1], None)):
        with pytest.raises(fa.FinitoError) as e:
            p.labels(lb, n_lab)
        assert e.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:
        lab.add(b, min_permille=1001)
    assert e.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:   # no replica on that device
        fa.FinimizerIndex.build(unitigs[:5], 31).labels(np.zeros(5, dtype=np.uint32))
    assert e.value.code == fa.FIN_ENODEV
    # a labelling of another index
    p2 = fa.FinimizerIndex.build(unitigs, 31).to_device(0)
    foreign = p2.labels(labels)
    for call in (lambda: b.classify(foreign), lambda: foreign.add(b), lambda: p.classify_reads(reads[:10], foreign)):
        with pytest.raises(fa.FinitoError) as e:
            call()
        assert e.value.code == fa.FIN_EINVAL
    bases, offsets = fa.flatten(reads[:10])
    err = fa.C.create_string_buffer(512)
    assert fa.lib().fin_search_batch_add_classes(p.h, bases.ctypes.data_as(fa.C.c_char_p), offsets.ctypes.data_as(fa.C.POINTER(fa.C.c_uint64)), 10, fa.FIN_MERGED, foreign.h,
                                                 1, 0, 0, err, 512) == fa.FIN_EINVAL and b"another index" in err.value
    assert foreign.download()[1] == 0
    foreign.close(); p2.close()
    # a batch that has not run
    b2 = p.batch(reads[:10])
    for call in (lambda: b2.classify(lab), lambda: lab.add(b2)):
        with pytest.raises(fa.FinitoError) as e:
            call()
        assert e.value.code == fa.FIN_EINVAL
    assert b2.device_read_classes_ptr() == 0
    b2.close(); b.close(); lab.close()


@pytest.mark.parametrize("n_reads", [1, 64 * 4 + 1, None])
def test_tally(n_reads, set31):
    """one atomic add per distinct slot per wave: a batch of one read, one of 64 * 4 + 1 reads (a whole block and one lane of the next), the whole set"""
    p, o, unitigs, labels, reads, nks, want = set31
    n = len(reads) if n_reads is None else n_reads
    reads, nks, want = reads[:n], nks[:n], want[:n]
    lab = p.labels(labels)
    b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
    for rule in RULES:
        w = tally_of(want, nks, 7, *rule)
        if n_reads is None:   # conditions on the input: every rule assigns some reads and leaves some; a margin of 1 leaves the ties
            assert 0 < w[-1] < n
        assert b.device_read_classes_ptr() == 0 or rule != RULES[0]
        tally, total = lab.reset().add(b, *rule).download()   # (the first add makes the classes)
        assert tally.dtype == np.uint64 and np.array_equal(tally, w) and total == n == int(tally.sum()), "%d reads, rule %s: got %s, want %s" % (n, rule, tally, w)
        tally, total = lab.add(b, *rule).download()           # adding twice counts twice
        assert np.array_equal(tally, 2 * w) and total == 2 * n
        assert lab.reset().download()[1] == 0
    if n_reads is None:
        assert tally_of(want, nks, 7, 1, 0, 0)[-1] < tally_of(want, nks, 7, 1, 0, 1)[-1]
    assert_classes(b.classify(lab), want, "%d reads: the classes after the adds" % n)
    b.close(); lab.close()


def test_host_buffers_in_many_sub_batches(set31):
    p, o, unitigs, labels, reads, nks, want = set31
    lab = p.labels(labels)
    got1 = p.classify_reads(reads, lab)
    assert_classes(got1, want, "one batch")
    tally1 = {rule: lab.reset().add_reads(reads, *rule).download() for rule in RULES}
    for rule in RULES:
        assert np.array_equal(tally1[rule][0], tally_of(want, nks, 7, *rule)) and tally1[rule][1] == len(reads), "one batch, rule %s" % (rule,)
    n_kmers = int(nks.sum())
    for sub, depth in ((n_kmers // 6, 3), (20000, 1), (500, 8)):
        p.set_option("max_batch_kmers", sub); p.set_option("pipeline_depth", depth)
        try:
            got = p.classify_reads(reads, lab)
            tally = {rule: lab.reset().add_reads(reads, *rule).download() for rule in RULES}
        finally:
            p.set_option("max_batch_kmers", None); p.set_option("pipeline_depth", None)
        assert n_kmers // sub >= 3   # at least three sub-batches
        assert_classes(got, got1, "sub-batches of %d k-mers" % sub)
        for rule in RULES:
            assert np.array_equal(tally[rule][0], tally1[rule][0]) and tally[rule][1] == len(reads), "sub-batches of %d k-mers, rule %s" % (sub, rule)
    for rd in ([], ["", "ACG"]):
        got = p.classify_reads(rd, lab)
        assert len(got) == len(rd) and (got["label"] == NONE).all()
        assert lab.reset().add_reads(rd).download()[1] == len(rd)
    with pytest.raises(fa.FinitoError) as e:
        lab.add_reads(reads[:10], min_permille=1001)
    assert e.value.code == fa.FIN_EINVAL
    lab.close()


def test_unitig_numbers(set31):
    p, o, unitigs, labels, reads, nks, want = set31
    k = 31
    want_numbers = numbers_of(unitigs, k)
    got = p.unitig_numbers(unitigs)
    assert got.dtype == np.uint32 and np.array_equal(got, want_numbers) and np.array_equal(np.sort(got), np.arange(len(unitigs)))
    # the numbers are the ones the pairs carry: a unitig searched as a read is found in the unitig of its number, from offset 0 on
    first = oracle_pairs(o, unitigs[:30], fa.FIN_FWD)[np.concatenate([[0], np.cumsum(nks_of(unitigs[:30], k))])[:-1]]
    assert np.array_equal(first, np.stack([want_numbers[:30], np.zeros(30, np.int64)], axis=1))
    assert len(p.unitig_numbers([])) == 0 and np.array_equal(p.unitig_numbers(unitigs[5:7] + unitigs[5:6]), want_numbers[[5, 6, 5]])
    inside = next(u for u in unitigs if len(u) > k + 5)
    for bad, word in ((unitigs[:3] + [unitigs[3][:k - 1]], "sequence 3"), ([unitigs[0], inside[2:]], "sequence 1"), ([random_genome(np.random.default_rng(3), 60)], "sequence 0")):
        with pytest.raises(fa.FinitoError) as e:   # shorter than k; begins inside a unitig; not in the index at all
            p.unitig_numbers(bad)
        assert e.value.code == fa.FIN_EINVAL and word in str(e.value)


def test_a_withheld_step_has_no_classes_and_tallies_nothing():
    """a step whose overflow list overran (tests/test_segments.py::test_a_withheld_step_has_no_segments' recipe) has no results: classify and Labels.add -- which
    makes the classes -- report FIN_ELIMIT, no class is written and the tally stays empty; a good step tallied afterwards is exact"""
    from tests.util import sample_reads
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    reads = sample_reads(rng, g, 500, 150)
    nks = nks_of(reads, k)
    labels = run_labelling(rng, len(unitigs))
    want = classes_of(oracle_pairs(o, reads), nks, labels)
    L = fa.lib()
    lab = p.labels(labels)
    try:
        assert L.fin_set_option(b"lds_deque_limit", 1) == 0 and L.fin_set_option(b"seed_anchors", 0) == 0 and L.fin_set_option(b"debug_ovf_cap", 3) == 0
        for mode in (0, 2):
            for first in (lambda: lab.add(b), lambda: b.classify(lab)):   # either may be the first to look at the step's overflow counter
                b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
                for call in (first, lambda: lab.add(b), lambda: b.classify(lab)):
                    with pytest.raises(fa.FinitoError) as e:
                        call()
                    assert e.value.code == fa.FIN_ELIMIT and "overflow list" in str(e.value)
                assert b.device_read_classes_ptr() == 0
                tally, total = lab.download()
                assert total == 0 and not tally.any(), "a withheld step was tallied (mode %d)" % mode
                b.close()
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        tally, total = lab.add(b).download()
        assert np.array_equal(tally, tally_of(want, nks, lab.n_labels, 1, 0, 0)) and total == len(reads), "a good step afterwards"
        assert_classes(b.classify(lab), want, "a good step afterwards")
        b.close()
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)
        lab.close(); p.close()
