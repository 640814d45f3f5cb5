"""Colour sets per unitig and read pseudoalignment, on the device (include/finito_amd.h: fin_colors_*, fin_batch_add_colors, fin_batch_pseudoalign,
fin_search_batch_add_colors, fin_search_batch_pseudoalign; fin_colors.hip).  The expectation is always the definition written in numpy
(tests/test_colors_host.py::rows_of) over the ORACLE's pairs -- or, for hand-made pairs, over those pairs -- never a device output or a fin_records_* result;
every comparison is exact."""
import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.test_colors_host import assert_pseudo, pack, pack_members, random_matrix, rows_of, unpack, words_of
from tests.test_read_class import numbers_of
from tests.test_read_class_host import assert_classes, classes_of, run_labelling
from tests.test_read_summary_host import assert_summaries, summaries_of
from tests.test_records_device import inject
from tests.test_segments import nks_of, oracle_pairs
from tests.test_segments_host import assert_segments, segments_of
from tests.test_unitig_counts import read_families
from tests.util import cut_unitigs, hand_made_case, random_genome

pytestmark = pytest.mark.gpu

PERMILLES = (0, 300, 1000)


def hand_picked(unitigs, k, bits, n_colors):
    """four unitigs given rows of their own -- a {0}, b {last colour}, c {0 and the last colour} (n_colors > 1), d {} -- and the reads made of them: two unitigs with
    disjoint colour sets joined, two with overlapping sets, an uncoloured unitig alone, coloured + uncoloured.  Returns (the matrix, the reads)"""
    num = numbers_of(unitigs, k)
    a, b, c, d = [i for i in range(len(unitigs)) if len(unitigs[i]) >= k + 20][:4]
    bits = np.array(bits)
    top = n_colors - 1
    for i, cs in ((a, [0]), (b, [top]), (c, [0, top]), (d, [])):
        bits[num[i]] = pack([cs], n_colors)[0]
    m = min(len(unitigs[i]) for i in (a, b, c, d))
    return bits, [unitigs[a][:m] + unitigs[b][:m], unitigs[a][:m] + unitigs[c][:m], unitigs[d], unitigs[a][:m] + unitigs[d][:m]]


def assert_expectation_shows_everything(want, n_colors):
    """want: {permille: (rows, heads)}"""
    h = want[1000][1]
    if n_colors > 1:
        assert ((want[1000][1]["n_colors"] == 0) & (want[0][1]["n_colors"] > 0)).any(), "no read with an empty intersection and a non-empty union"
        differ = (want[300][0] != want[0][0]).any(axis=1) & (want[300][0] != want[1000][0]).any(axis=1)
        assert differ.any(), "no read where 300 differs from 0 and from 1000"
    assert ((h["n_colored"] > 0) & (h["n_colored"] < h["n_found"])).any(), "no read with coloured and uncoloured found k-mers"
    assert ((h["n_found"] > 0) & (h["n_colored"] == 0)).any(), "no read whose found k-mers are all uncoloured"
    if n_colors & 63 != 1:
        assert (want[0][0][:, -1] >> np.uint64(1)).any(), "no set bit in the last word above bit 0"
    else:
        assert want[0][0][:, -1].any(), "no set bit in the last word"


@pytest.mark.parametrize("k", [16, 31, 63, 127])
def test_pseudoalignment_of_every_read_family_in_every_text_mode(k):
    """text modes 0, 1 and 2 under matrices of 5, 64, 65 and 130 colours (W = 1, the 64/65 word edge, W = 3): in modes 1 and 2 the fast path's reads are row
    copies made from their records (in mode 2 their pairs do not exist); k = 127 leaves no records, every read goes through the pair scan.  The call changes
    neither segments nor summaries nor classes nor pairs"""
    rng = np.random.default_rng(1900 + k)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=max(700, 4 * k))
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    fam = read_families(rng, g, k, unitigs, n=800)
    mats, reads = {}, None
    for n_colors in (5, 64, 65, 130):
        mats[n_colors], picked = hand_picked(unitigs, k, random_matrix(rng, len(unitigs), n_colors), n_colors)
        reads = fam + picked
    nks = nks_of(reads, k)
    e1 = oracle_pairs(o, reads)
    want = {n: {pm: rows_of(e1, nks, mats[n], n, pm) for pm in PERMILLES} for n in mats}
    for n in mats:
        assert_expectation_shows_everything(want[n], n)
    labels = run_labelling(rng, len(unitigs))
    want_segs, want_sums, want_cls = segments_of(e1, nks), summaries_of(e1, nks), classes_of(e1, nks, labels)
    found = int((e1[:, 0] != -1).sum())
    cols = {n: p.colors(n, mats[n]) for n in mats}
    lab = p.labels(labels)
    assert cols[130].words == 3 and cols[64].words == 1 and cols[65].words == 2 and all(c.device_ptr() for c in cols.values())
    for n in mats:
        got, n_set = cols[n].download()
        assert np.array_equal(got, mats[n]) and n_set == int(unpack(mats[n], n).sum())
    for mode in (0, 1, 2):
        b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        assert b.device_pseudo_ptrs() == (0, 0)
        for n in mats:
            for pm in PERMILLES:
                assert_pseudo(b.pseudoalign(cols[n], pm), want[n][pm], "k=%d text mode %d, %d colours, permille %d" % (k, mode, n, pm))
        assert all(b.device_pseudo_ptrs())
        info = b.run_info()
        if k <= 63:
            assert info["fast_path"] and (mode == 0 or b.pipeline_counts()[41] > 0)   # the record path was really taken (modes 1 and 2)
        else:
            assert not info["fast_path"] and b.pipeline_counts()[41] == 0   # no records: every read goes through the scan
        assert_pseudo(b.pseudoalign(cols[130]), want[130][1000], "k=%d text mode %d, a first call" % (k, mode))
        assert_pseudo(b.pseudoalign(cols[130]), want[130][1000], "k=%d text mode %d, a second call" % (k, mode))
        assert_pseudo(b.pseudoalign(cols[5]), want[5][1000], "k=%d text mode %d, another matrix" % (k, mode))
        assert_pseudo(b.pseudoalign(cols[130]), want[130][1000], "k=%d text mode %d, the first matrix again" % (k, mode))
        # everything else the batch gives is what it gives without the call
        assert_segments(b.segments(), want_segs, "k=%d text mode %d, segments after the rows" % (k, mode))
        assert_summaries(b.read_summaries(), want_sums, "k=%d text mode %d, summaries after the rows" % (k, mode))
        assert_classes(b.classify(lab), want_cls, "k=%d text mode %d, classes after the rows" % (k, mode))
        if mode == 2 and info["fast_path"]:
            with pytest.raises(fa.FinitoError):
                b.download()
        else:
            pairs, npos = b.download()
            assert npos == found and np.array_equal(pairs.astype(np.int64), e1)
        assert_pseudo(b.pseudoalign(cols[65], 300), want[65][300], "k=%d text mode %d, after segments, summaries, classes and download" % (k, mode))
        b.reload(reads[:50])
        with pytest.raises(fa.FinitoError) as e:   # reloaded, not run yet
            b.pseudoalign(cols[5])
        assert e.value.code == fa.FIN_EINVAL and b.device_pseudo_ptrs() == (0, 0)
        b.close()
    for c in cols.values():
        c.close()
    lab.close(); p.close()


@pytest.fixture(scope="module")
def set31():
    rng = np.random.default_rng(21900)
    k = 31
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=700)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    reads = read_families(rng, g, k, unitigs, n=800)
    nks = nks_of(reads, k)
    pairs = oracle_pairs(o, reads)
    for a in (nks, pairs):
        a.setflags(write=False)
    yield p, o, g, unitigs, reads, nks, pairs, rng
    p.close()


def test_a_matrix_of_4096_colours(set31):
    """W = 64: the full-width row copy, a lane per word, and a 64-word reduction for the scanned reads"""
    p, o, g, unitigs, reads, nks, pairs, rng = set31
    n_colors = 4096
    bits, picked = hand_picked(unitigs, 31, random_matrix(rng, len(unitigs), n_colors), n_colors)
    rd = reads[:200] + picked
    e1, nk = oracle_pairs(o, rd), nks_of(rd, 31)
    col = p.colors(n_colors, bits)
    assert col.words == 64
    for mode in (0, 2):
        b = p.batch(rd); b.text_mode(mode); b.run(fa.FIN_MERGED)
        for pm in PERMILLES:
            want = rows_of(e1, nk, bits, n_colors, pm)
            if pm == 1000:
                assert (want[0][:, -1] >> np.uint64(63)).any() and (want[1]["n_colors"] > 64).any()
            assert_pseudo(b.pseudoalign(col, pm), want, "4096 colours, mode %d, permille %d" % (mode, pm))
        b.close()
    col.close()


@pytest.fixture(scope="module")
def wide():
    """an index of more than 200 unitigs for hand-made pairs"""
    k = 31
    rng = np.random.default_rng(1964)
    g = random_genome(rng, 12000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, k, max_len=80), k).to_device(0)
    assert p.n_unitigs >= 200
    yield p, rng
    p.close()


def walk(rng, us):
    """slots that walk through the unitigs `us` in stretches of 1 to 3, absent slots strewn in"""
    out = []
    for u in us:
        out += [(int(u), i) for i in range(int(rng.integers(1, 4)))]
        if rng.random() < 0.1:
            out.append((-1, -1))
    return out


@pytest.mark.parametrize("n_colors", [40, 130])
def test_reads_with_more_unitigs_than_the_table_holds_and_row_edges(wide, n_colors):
    """hand-made pairs (set_pairs, text mode 0: every read is scanned).  64 distinct unitigs fill the wave's table; 65, 70, 128 and 129 overflow it and the read is
    rescanned word by word -- the rows stay exact.  Reads of 0, 1, 63, 64, 65, 128 and 129 slots; a unitig number at or above n_unitigs is an absent slot"""
    p, rng = wide
    k, nu = 31, p.n_unitigs
    A = (-1, -1)
    cases = {}
    for n in (64, 65, 70, 128, 129):
        us = [int(u) for u in rng.permutation(nu)[:n]]
        cases["%d unitigs" % n] = walk(rng, us) + walk(rng, us[::-1][: n // 2])   # half of them twice: a repeated unitig adds to its count
        assert len({u for u, _ in cases["%d unitigs" % n] if u >= 0}) == n
    cases["200 unitigs"] = walk(rng, range(200))
    cases["64 unitigs, then absent slots"] = [(u, 0) for u in range(64)] + [A] * 70
    for nk in (0, 1, 63, 64, 65, 128, 129):
        cases["%d slots, one unitig" % nk] = [(5, i) for i in range(nk)]
        cases["%d slots, nothing" % nk] = [A] * nk
        cases["%d slots, the last one only" % nk] = [A] * max(nk - 1, 0) + [(11, 0)] * min(nk, 1)
        cases["%d slots, two unitigs" % nk] = [(7, i) for i in range(nk // 2)] + [(9, i) for i in range(nk - nk // 2)]
        cases["%d slots, a unitig outside the index" % nk] = [(nu, 0), (nu + 5, 1), (0x7FFFFFFF, 0), (-2, 0), (3, 1)][: nk] + [(3, 0)] * max(nk - 5, 0)
    names = list(cases)
    assert all(len(cases["%d unitigs" % n]) >= 200 for n in (128, 129)) and len(cases["70 unitigs"]) >= 170
    pairs = np.array([x for n in names for x in cases[n]], dtype=np.int32).reshape(-1, 2)
    nks = np.array([len(cases[n]) for n in names])
    reads = [random_genome(rng, int(nk) + k - 1) if nk else "ACGT" for nk in nks]
    bits = random_matrix(rng, nu, n_colors, empty_share=0.15)
    b = p.batch(reads); b.text_mode(0); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(pairs)
    col = p.colors(n_colors, bits)
    b.pseudoalign(col)
    b.set_pairs(pairs)
    assert b.device_pseudo_ptrs() == (0, 0)   # forgotten
    for pm in (0, 300, 500, 1000):
        want = rows_of(pairs, nks, bits, n_colors, pm)
        w = dict(zip(names, want[1].tolist()))
        assert w["129 slots, a unitig outside the index"][0] == 125 and w["1 slots, a unitig outside the index"][0] == 0
        rows, heads = b.pseudoalign(col, pm)
        for i, n in enumerate(names):
            assert tuple(heads[i].tolist()) == tuple(want[1][i].tolist()) and np.array_equal(rows[i], want[0][i]), \
                "%s, %d colours, permille %d: got %s %s, want %s %s" % (n, n_colors, pm, heads[i], rows[i], want[1][i], want[0][i])
    # a colour per unitig: the union of a read of 129 unitigs has 129 colours (W = 4)
    one_each = pack([[u] for u in range(nu)], nu)
    col2 = p.colors(nu, one_each)
    want = rows_of(pairs, nks, one_each, nu, 0)
    assert want[1]["n_colors"][names.index("129 unitigs")] == 129
    assert_pseudo(b.pseudoalign(col2, 0), want, "a colour per unitig, the union")
    assert_pseudo(b.pseudoalign(col2, 1000), rows_of(pairs, nks, one_each, nu, 1000), "a colour per unitig, the intersection")
    # colouring by these pairs: every unitig met, and no other, gets the colour
    col2.reset().add(b, 7)
    got, n_set = col2.download()
    met = np.unique(pairs[(pairs[:, 0] >= 0) & (pairs[:, 0] < nu), 0])
    want_bits = np.zeros_like(one_each); want_bits[met, 0] = 1 << 7
    assert np.array_equal(got, want_bits) and n_set == len(met)
    b.close(); col.close(); col2.close()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("k", [16, 63])
def test_hand_made_records_on_the_device(k, mode):
    """the whole record format through the kind-1 branch: coloured and uncoloured unitigs, no found slot after the gaps, kind 2, both strands, all three kinds in
    every wave; in mode 2 a finished read's pair slots hold garbage, which nobody may read"""
    c = hand_made_case(k)
    rng = np.random.default_rng(1950 + k)
    p = fa.FinimizerIndex.build(c.unitigs, k).to_device(0)
    b = p.batch(c.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(c.pairs)
    inject(b, c.recs, c.pairs, mode)
    for n_colors in (1, 65):
        bits = random_matrix(rng, len(c.unitigs), n_colors)
        col = p.colors(n_colors, bits)
        for pm in PERMILLES:
            assert_pseudo(b.pseudoalign(col, pm), rows_of(c.pairs, c.nks, bits, n_colors, pm), "k=%d text mode %d, %d colours, permille %d" % (k, mode, n_colors, pm))
        got, n_set = col.reset().add(b, n_colors - 1).download()
        met = np.unique(c.pairs[c.pairs[:, 0] >= 0, 0])
        want_bits = np.zeros_like(bits); want_bits[met, -1] = np.uint64(1) << np.uint64((n_colors - 1) & 63)
        assert np.array_equal(got, want_bits) and n_set == len(met), "k=%d text mode %d: colouring from records" % (k, mode)
        col.close()
    b.close(); p.close()


def references_of(g, n=5):
    """n overlapping stretches of the genome; its end is in none of them"""
    step = len(g) // (n + 2)
    return [g[i * step: (i + 2) * step] for i in range(n)]


def brute_colours(o, refs, n_unitigs, n_colors, colors=None):
    """unitig u has colour i iff the oracle finds some k-mer of reference i in u"""
    member = np.zeros((n_unitigs, n_colors), dtype=np.uint8)
    for i, ref in enumerate(refs):
        e = oracle_pairs(o, [ref])
        member[np.unique(e[e[:, 0] >= 0, 0]), i if colors is None else colors[i]] = 1
    return pack_members(member)


def test_colouring_by_search(set31):
    p, o, g, unitigs, reads, nks, pairs, rng = set31
    refs = references_of(g)
    nu = p.n_unitigs
    want = brute_colours(o, refs, nu, 5)
    shared = unpack(want, 5).sum(axis=1)
    assert (shared == 1).any() and (shared == 2).any() and (shared == 0).sum() > 0 and want[:, 0].max() >= 16   # unitigs of one reference, shared ones, untouched ones
    col = p.colors(5)
    assert col.download()[1] == 0
    # every reference cut into windows of 1000 k-mers that overlap by k - 1 bases: no k-mer is lost
    windows = lambda s: [s[a: a + 1000 + 30] for a in range(0, len(s) - 30, 1000)]
    for i, ref in enumerate(refs):
        col.add_reads(windows(ref), i)
    got, n_set = col.download()
    assert np.array_equal(got, want) and n_set == int(unpack(want, 5).sum()), "host buffers"
    for i, ref in enumerate(refs):   # adding twice changes nothing
        col.add_reads([ref], i)
    assert np.array_equal(col.download()[0], want)
    assert col.reset().download()[1] == 0 and not col.download()[0].any()
    for mode in (0, 2):
        col.reset()
        for i, ref in enumerate(refs):
            b = p.batch(windows(ref)); b.text_mode(mode); b.run(fa.FIN_MERGED)
            col.add(b, i).add(b, i)
            b.close()
        got, n_set = col.download()
        assert np.array_equal(got, want) and n_set == int(unpack(want, 5).sum()), "Colors.add, text mode %d" % mode
    col.close()
    # colour 63 and colour 64 of a 130-colour matrix land in the right words
    col = p.colors(130)
    for i, c in enumerate((63, 64, 129, 0, 65)):
        col.add_reads([refs[i]], c)
    got, n_set = col.download()
    want130 = brute_colours(o, refs, nu, 130, colors=(63, 64, 129, 0, 65))
    assert got.shape == (nu, 3) and np.array_equal(got, want130) and n_set == int(unpack(want130, 130).sum())
    assert (got[:, 0] >> np.uint64(63)).any() and (got[:, 1] & np.uint64(1)).any() and (got[:, 2] == 2).any()
    col.close()


def test_host_buffers(set31):
    p, o, g, unitigs, reads, nks, pairs, rng = set31
    n_colors = 70
    bits, picked = hand_picked(unitigs, 31, random_matrix(rng, len(unitigs), n_colors), n_colors)
    rd = reads + picked
    nk = nks_of(rd, 31)
    col = p.colors(n_colors, bits)
    for strands in (fa.FIN_MERGED, fa.FIN_FWD):
        e = oracle_pairs(o, rd, strands)
        for pm in (1000, 300):
            want = rows_of(e, nk, bits, n_colors, pm)
            rows, heads, npos = p.pseudoalign_reads(rd, col, pm, strands)
            assert_pseudo((rows, heads), want, "host buffers, strands %d, permille %d" % (strands, pm))
            assert npos == int(want[1]["n_colored"].sum()) > 0
    want = rows_of(oracle_pairs(o, rd), nk, bits, n_colors, 1000)
    n_kmers = int(nk.sum())
    p.set_option("max_batch_kmers", n_kmers // 6); p.set_option("pipeline_depth", 3)
    try:
        rows, heads, npos = p.pseudoalign_reads(rd, col)
        none, heads2, npos2 = p.pseudoalign_reads(rd, col, want_rows=False)
    finally:
        p.set_option("max_batch_kmers", None); p.set_option("pipeline_depth", None)
    assert_pseudo((rows, heads), want, "host buffers, six sub-batches")
    assert none is None and heads2.tobytes() == want[1].tobytes() and npos == npos2 == int(want[1]["n_colored"].sum())
    for empty in ([], ["", "ACG"]):
        rows, heads, npos = p.pseudoalign_reads(empty, col)
        assert rows.shape == (len(empty), 2) and len(heads) == len(empty) and npos == 0 and not rows.any() and not heads["n_found"].any()
        col.add_reads(empty, 3)
    assert np.array_equal(col.download()[0], bits)
    with pytest.raises(fa.FinitoError) as e:
        p.pseudoalign_reads(rd[:10], col, 1001)
    assert e.value.code == fa.FIN_EINVAL
    col.close()


def test_colour_by_search_then_pseudoalign(set31):
    """error-free reads drawn from one reference each: the intersection over a read's coloured k-mers contains the colour of its source, by construction"""
    p, o, g, unitigs, reads, nks, pairs, rng = set31
    refs = references_of(g)
    col = p.colors(5)
    for i, ref in enumerate(refs):
        col.add_reads([ref], i)
    bits = col.download()[0]
    src = rng.integers(0, 5, 400)
    rd = []
    for i in src:
        a = int(rng.integers(0, len(refs[i]) - 150))
        rd.append(refs[i][a: a + 150])
    rows, heads, npos = p.pseudoalign_reads(rd, col)
    assert_pseudo((rows, heads), rows_of(oracle_pairs(o, rd), nks_of(rd, 31), bits, 5, 1000), "coloured by search")
    assert ((rows[:, 0] >> src.astype(np.uint64)) & np.uint64(1)).all() and (heads["n_colored"] == heads["n_found"]).all() and (heads["n_found"] > 0).all()
    assert (heads["n_colors"] == 1).any() and (heads["n_colors"] == 2).any()   # reads from a stretch one reference has alone, reads from an overlap
    col.close()


def test_refusals_on_the_device(set31):
    p, o, g, unitigs, reads, nks, pairs, rng = set31
    col = p.colors(5)
    b = p.batch(reads[:50])
    for call in (lambda: b.pseudoalign(col), lambda: col.add(b, 0)):   # a batch that has not run
        with pytest.raises(fa.FinitoError) as e:
            call()
        assert e.value.code == fa.FIN_EINVAL
    assert b.device_pseudo_ptrs() == (0, 0)
    b.run(fa.FIN_MERGED)
    err = fa.C.create_string_buffer(512)
    for color in (5, 64, 0xFFFFFFFF):   # a colour at or above n_colors
        assert fa.lib().fin_batch_add_colors(b.h, col.h, color, None, err, 512) == fa.FIN_EINVAL and b"n_colors" in err.value
        with pytest.raises(fa.FinitoError) as e:
            col.add(b, color)
        assert e.value.code == fa.FIN_EINVAL
    bases, offsets = fa.flatten(reads[:10])
    assert fa.lib().fin_search_batch_add_colors(p.h, bases.ctypes.data_as(fa.C.c_char_p), offsets.ctypes.data_as(fa.C.POINTER(fa.C.c_uint64)), 10, fa.FIN_MERGED, col.h, 5,
                                                err, 512) == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:
        b.pseudoalign(col, 1001)
    assert e.value.code == fa.FIN_EINVAL
    assert col.download()[1] == 0
    # colours of another index
    p2 = fa.FinimizerIndex.build(unitigs, 31).to_device(0)
    foreign = p2.colors(5)
    for call in (lambda: b.pseudoalign(foreign), lambda: foreign.add(b, 0), lambda: p.pseudoalign_reads(reads[:10], foreign)):
        with pytest.raises(fa.FinitoError) as e:
            call()
        assert e.value.code == fa.FIN_EINVAL
    assert fa.lib().fin_search_batch_add_colors(p.h, bases.ctypes.data_as(fa.C.c_char_p), offsets.ctypes.data_as(fa.C.POINTER(fa.C.c_uint64)), 10, fa.FIN_MERGED, foreign.h, 0,
                                                err, 512) == fa.FIN_EINVAL and b"another index" in err.value
    assert foreign.download()[1] == 0
    # what upload refuses: a set bit at or above n_colors (the message names the unitig), a matrix of another shape
    bad = np.zeros((p.n_unitigs, 1), dtype=np.uint64); bad[17, 0] = 1 << 5
    with pytest.raises(fa.FinitoError) as e:
        col.upload(bad)
    assert e.value.code == fa.FIN_EINVAL and "unitig 17" in str(e.value)
    with pytest.raises(fa.FinitoError) as e:
        col.upload(bad[:-1])
    assert e.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:   # no replica on that device
        fa.FinimizerIndex.build(unitigs[:5], 31).colors(5)
    assert e.value.code == fa.FIN_ENODEV
    foreign.close(); p2.close(); b.close(); col.close()


def test_a_withheld_step_colours_nothing_has_no_rows_and_is_reported_until_the_reset():
    """a step whose overflow list overran (tests/test_unitig_coverage.py::test_a_withheld_step_sets_nothing_and_is_reported_until_the_reset's recipe) has no
    results: Colors.add reads the counter itself, sets no bit and flags the matrix -- fin_colors_download reports FIN_ELIMIT until the reset --, pseudoalign
    reports FIN_ELIMIT and writes no row; after the reset the matrix is clean and a good step coloured and pseudoaligned is exact"""
    from tests.util import sample_reads
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    reads = sample_reads(rng, g, 500, 150)
    e1 = oracle_pairs(o, reads)
    member = np.zeros((p.n_unitigs, 5), dtype=np.uint8); member[np.unique(e1[e1[:, 0] >= 0, 0]), 3] = 1
    want = pack_members(member)
    L = fa.lib()
    col, other = p.colors(5), p.colors(5, random_matrix(rng, len(unitigs), 5))
    try:
        assert L.fin_set_option(b"lds_deque_limit", 1) == 0 and L.fin_set_option(b"seed_anchors", 0) == 0 and L.fin_set_option(b"debug_ovf_cap", 3) == 0
        for mode in (0, 2):
            b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
            col.add(b, 3)                              # nobody has looked at the step's overflow counter yet: the kernel does
            with pytest.raises(fa.FinitoError) as e:
                col.download()
            assert e.value.code == fa.FIN_ELIMIT and "overflow list" in str(e.value)
            with pytest.raises(fa.FinitoError) as e:   # ... and keeps saying so
                col.download()
            assert e.value.code == fa.FIN_ELIMIT
            bits, n_set = col.reset().download()
            assert n_set == 0 and not bits.any(), "a withheld step set colours (mode %d)" % mode
            with pytest.raises(fa.FinitoError) as e:
                b.pseudoalign(other)
            assert e.value.code == fa.FIN_ELIMIT and "overflow list" in str(e.value) and b.device_pseudo_ptrs() == (0, 0)
            with pytest.raises(fa.FinitoError) as e:   # once the host knows, the add itself refuses
                col.add(b, 3)
            assert e.value.code == fa.FIN_ELIMIT and col.download()[1] == 0
            b.close()
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        bits, n_set = col.add(b, 3).download()
        assert np.array_equal(bits, want) and n_set == int(member.sum()) > 0, "a good step after the reset"
        assert_pseudo(b.pseudoalign(col), rows_of(e1, nks_of(reads, k), want, 5, 1000), "a good step after the reset")
        b.close()
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)
        col.close(); other.close(); p.close()
