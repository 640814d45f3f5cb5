"""Equivalence classes of pseudoaligned reads, accumulated on the device (include/finito_amd.h: fin_eqclasses_*, fin_batch_add_eqclasses,
fin_search_batch_add_eqclasses; fin_eqclasses.hip).  The expectation is always the definition in numpy -- np.unique(rows, axis=0, return_counts=True) over the
non-empty rows (tests/test_eqclasses_host.py::classes_of_rows) that tests/test_colors_host.py::rows_of gives on the ORACLE's pairs or on hand-made pairs, or over
hand-made rows -- never a device output or a fin_rows_eqclasses result; every comparison is exact."""
import numpy as np
import pytest
import torch

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.test_colors import hand_picked
from tests.test_colors_host import pack, random_matrix, rows_of, words_of
from tests.test_eqclasses_host import assert_classes, classes_of_rows, random_rows, tally_of
from tests.test_eqclasses_table_host import tags_of
from tests.test_read_summary_host import assert_summaries, summaries_of
from tests.test_segments import nks_of, oracle_pairs
from tests.test_segments_host import assert_segments, segments_of
from tests.test_unitig_counts import read_families
from tests.util import cut_unitigs, random_genome, sample_reads

pytestmark = pytest.mark.gpu


def times(want, n):
    return want[0], want[1] * np.uint64(n), want[2] * n


def assert_all(eq, want, n_colors, what, n_rows=None):
    """download, tally and the first three stats against the definition"""
    assert_classes(eq.download(), want, what)
    w, o, un = eq.tally()
    ww, wo = tally_of(want[0], want[1], n_colors)
    assert np.array_equal(w, ww) and np.array_equal(o, wo) and un == want[2], what + ": the tally"
    st = eq.stats()
    assert st[:3] == [int(want[1].sum()) + want[2], want[2], len(want[0])], "%s: stats %s" % (what, st)
    if n_rows is not None:
        assert st[0] == n_rows, what


def on_device(rows):
    t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return t


def keep_one_of_the_smallest_class(rows):
    """a mask over the reads: every read stays but those of the smallest class (by the definition's rows) behind its first"""
    live = np.nonzero(rows.any(axis=1))[0]
    _, inv, cnt = np.unique(rows[live], axis=0, return_inverse=True, return_counts=True)
    keep = np.ones(len(rows), dtype=bool)
    keep[live[np.asarray(inv).reshape(-1) == int(np.argmin(cnt))][1:]] = False
    return keep


# ---- 1. read families ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [16, 31, 127])
def test_read_families_in_text_modes_0_and_2(k):
    rng = np.random.default_rng(2200 + k)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=max(700, 4 * k))
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    fam = read_families(rng, g, k, unitigs, n=800)
    mats, reads = {}, None
    for n_colors in (5, 65, 130):
        mats[n_colors], picked = hand_picked(unitigs, k, random_matrix(rng, len(unitigs), n_colors), n_colors)
        reads = fam + picked
    a = [i for i in range(len(unitigs)) if len(unitigs[i]) >= k + 20][0]   # hand_picked's unitig a, whose row is {0}: a class of more than 64 reads
    reads = reads + [unitigs[a][j % 10: j % 10 + k + 10] for j in range(70)]
    nks = nks_of(reads, k)
    e1 = oracle_pairs(o, reads)
    at = np.concatenate([[0], np.cumsum(nks)])
    for n_colors in mats:
        col = p.colors(n_colors, mats[n_colors])
        eq = col.eqclasses(4096)
        for pm in (1000, 0):
            # the expectation must show a class of one read: of the smallest class of the definition's rows only the first read stays in the read set
            rows = rows_of(e1, nks, mats[n_colors], n_colors, pm)[0]
            keep = np.nonzero(keep_one_of_the_smallest_class(rows))[0]
            rd, nk = [reads[i] for i in keep], nks[keep]
            pairs = np.concatenate([e1[at[i]:at[i + 1]] for i in keep])
            want = classes_of_rows(rows[keep], n_colors)
            assert want[1].max() > 64 and (want[1] == 1).any() and want[2] > 0, "the expectation lacks a large class, a class of one read or unaligned reads"
            want_segs, want_sums = segments_of(pairs, nk), summaries_of(pairs, nk)
            found = int((pairs[:, 0] != -1).sum())
            for mode in (0, 2):
                what = "k=%d, %d colours, permille %d, text mode %d" % (k, n_colors, pm, mode)
                b = p.batch(rd); b.text_mode(mode); b.run(fa.FIN_MERGED)
                assert eq.reset().add(b, pm) is eq
                if k <= 63 and mode == 2:
                    assert b.pipeline_counts()[41] > 0   # the fast path's reads are row copies
                assert_all(eq, want, n_colors, what, n_rows=len(rd))
                eq.add(b, pm)
                assert_all(eq, times(want, 2), n_colors, what + ", added twice", n_rows=2 * len(rd))
                # everything else the batch gives is what it gives without the call
                assert_segments(b.segments(), want_segs, what + ", segments after the add")
                assert_summaries(b.read_summaries(), want_sums, what + ", summaries after the add")
                if mode == 0:
                    got, npos = b.download()
                    assert npos == found and np.array_equal(got.astype(np.int64), pairs)
                b.close()
        eq.close(); col.close()
    p.close()


# ---- 2. hand-made rows through add_rows ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(2290)
    k = 31
    g = random_genome(rng, 12000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, k, max_len=80), k).to_device(0)
    assert p.n_unitigs >= 200
    yield p, g, rng
    p.close()


N_COLORS_OF_W = {1: 40, 2: 100, 3: 130, 64: 4096 - 17}


@pytest.mark.parametrize("W", [1, 2, 3, 64])
def test_hand_made_rows(small, W):
    p, g, rng = small
    n_colors = N_COLORS_OF_W[W]
    assert words_of(n_colors) == W and n_colors & 63
    col = p.colors(n_colors)
    eq = col.eqclasses(1024)
    top = n_colors - 1
    one = lambda cs: pack([cs], n_colors)[0]
    zero = np.zeros(W, dtype=np.uint64)
    cases = {}
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        cases["%d rows" % n] = random_rows(rng, n, n_colors, 12) if n else np.zeros((0, W), dtype=np.uint64)
    cases["a wave of 64 equal rows"] = np.array([one([0, top])] * 64)
    cases["63 equal rows and one other"] = np.array([one([3])] * 37 + [one([3, top])] + [one([3])] * 26)
    cases["64 rows, all different"] = np.array([one([c for c in range(7) if (i + 1) >> c & 1] + [top]) for i in range(64)])
    assert len(np.unique(cases["64 rows, all different"], axis=0)) == 64
    cases["empty rows and classes lane by lane"] = np.array([zero if i % 2 else one([i % 6]) for i in range(192)])
    cases["classes and empty rows lane by lane"] = np.array([one([top - i % 5]) if i % 2 else zero for i in range(130)])
    cases["rows equal except in the last word"] = np.array([one([2, 3] + [[64 * (W - 1)], [64 * (W - 1) + 1], [64 * (W - 1), 64 * (W - 1) + 1]][i % 3]) for i in range(100)])
    assert W == 1 or len(np.unique(cases["rows equal except in the last word"][:, : W - 1], axis=0)) == 1
    assert len(np.unique(cases["rows equal except in the last word"], axis=0)) == 3
    for name, rows in cases.items():
        t = on_device(rows) if len(rows) else None
        eq.reset().add_rows(t.data_ptr() if len(rows) else 0, len(rows))
        assert_all(eq, classes_of_rows(rows, n_colors), n_colors, "W=%d, %s" % (W, name), n_rows=len(rows))
    # everything in one accumulator, add after add
    eq.reset()
    kept = [on_device(rows) for rows in cases.values() if len(rows)]   # (alive until the download has waited for the adds)
    for t in kept:
        eq.add_rows(t.data_ptr(), t.shape[0])
    assert_all(eq, classes_of_rows(np.concatenate(list(cases.values())), n_colors), n_colors, "W=%d, every case added" % W)
    # a stray bit at n_colors: FIN_EINVAL until the reset; without it the other rows of that add are exact
    good = cases["257 rows"]
    bad = good.copy(); bad[100] = one([0]); bad[100, W - 1] |= np.uint64(1) << np.uint64(n_colors & 63)
    t = on_device(bad)
    eq.reset().add_rows(t.data_ptr(), len(bad))
    for _ in range(2):
        with pytest.raises(fa.FinitoError) as e:
            eq.download()
        assert e.value.code == fa.FIN_EINVAL and "n_colors" in str(e.value)
    rest = np.delete(bad, 100, axis=0)
    t = on_device(rest)
    eq.reset().add_rows(t.data_ptr(), len(rest))
    assert_all(eq, classes_of_rows(rest, n_colors), n_colors, "W=%d, after the stray bit" % W, n_rows=len(rest))
    eq.close(); col.close()


# ---- 3. hand-made pairs through set_pairs ----------------------------------------------------------------------------------------------
def test_hand_made_pairs(small):
    p, g, rng = small
    k, nu, n_colors = 31, p.n_unitigs, 70
    # groups of unitigs share a row: unitig u has row u % 7 of seven rows, the last of them empty (uncoloured unitigs)
    group_rows = pack([[0], [1, 69], [0, 1], [2, 3, 64], [69], [0, 1, 2, 3], []], n_colors)
    bits = group_rows[np.arange(nu) % 7]
    reads_pairs = []
    for u in range(0, 150):                                     # one unitig
        reads_pairs.append([(u, i) for i in range(1 + u % 5)])
    for u in range(0, 60):                                      # two unitigs with different rows: the intersection and the union differ
        reads_pairs.append([(u, 0), (u, 1), (-1, -1), (u + 1, 0)])
    for u in range(6, 100, 7):                                  # uncoloured unitigs
        reads_pairs.append([(u, 0), (u, 1)])
    reads_pairs.append([(-1, -1)] * 3)
    nks = np.array([len(x) for x in reads_pairs])
    pairs = np.array([x for r in reads_pairs for x in r], dtype=np.int32).reshape(-1, 2)
    reads = [random_genome(rng, int(nk) + k - 1) for nk in nks]
    b = p.batch(reads); b.text_mode(0); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(pairs)
    b.set_pairs(pairs)
    col = p.colors(n_colors, bits)
    eq = col.eqclasses(64)
    want = {pm: classes_of_rows(rows_of(pairs, nks, bits, n_colors, pm)[0], n_colors) for pm in (0, 1000)}
    met = len(np.unique(pairs[pairs[:, 0] >= 0, 0]))
    assert len(want[1000][0]) < met and len(want[0][0]) < met and want[1000][2] > 14      # fewer classes than unitigs met
    assert len(want[0][0]) != len(want[1000][0]) or (want[0][0] != want[1000][0]).any()   # the threshold changes the classes
    for pm in (0, 1000):
        eq.reset().add(b, pm)
        assert_all(eq, want[pm], n_colors, "hand-made pairs, permille %d" % pm, n_rows=len(reads))
    eq.close(); col.close(); b.close()


# ---- 4. shared tags --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("tag_bits", [1, 4])
def test_rows_that_share_a_tag_go_through_the_serial_pass(small, W, tag_bits):
    p, g, rng = small
    n_colors = 64 * W
    col = p.colors(n_colors)
    pool = np.unique(rng.integers(1, 1 << 63, size=(300, W), dtype=np.uint64), axis=0)
    assert len(pool) == 300
    rows = pool[np.concatenate([np.arange(300), rng.integers(0, 300, 1700)])][rng.permutation(2000)]
    want = classes_of_rows(rows, n_colors)
    assert len(want[0]) == 300
    t = on_device(rows)
    p.set_option("ec_tag_bits", tag_bits)
    try:
        eq = col.eqclasses(1000)
        eq.add_rows(t.data_ptr(), len(rows))
        assert_all(eq, want, n_colors, "W=%d, %d tag bits" % (W, tag_bits), n_rows=2000)
        first = eq.stats()[3]
        assert first > 0
        eq.add_rows(t.data_ptr(), len(rows))   # rows that lost a tag reach their slot through the serial pass again
        assert_all(eq, times(want, 2), n_colors, "W=%d, %d tag bits, a second add" % (W, tag_bits), n_rows=4000)
        assert eq.stats()[3] > first
    finally:
        p.set_option("ec_tag_bits", None)
    eq.add_rows(t.data_ptr(), len(rows))       # the option cleared: the table built under narrow tags is still the table
    assert_all(eq, times(want, 3), n_colors, "W=%d, %d tag bits, a third add with the option cleared" % (W, tag_bits), n_rows=6000)
    # after a reset the full-width tags are back: nothing goes through the serial pass
    eq.reset().add_rows(t.data_ptr(), len(rows))
    assert_all(eq, want, n_colors, "W=%d, after the reset" % W, n_rows=2000)
    assert eq.stats()[3] == 0
    # the owners first: above, which row of a tag wins its slot is a race, so the figure is only positive.  With one row per tag in the table before the others
    # arrive, a row goes through the serial pass iff it is not its tag's owner row -- the exact figure, by the mirror of tests/test_eqclasses_table_host.py
    tags = tags_of(rows, tag_bits)
    owners = rows[np.sort(np.unique(tags, return_index=True)[1])]
    owner_of = {int(tg): r.tobytes() for tg, r in zip(tags_of(owners, tag_bits), owners)}
    serial = sum(1 for tg, r in zip(tags, rows) if owner_of[int(tg)] != r.tobytes())
    assert len(owners) == min(300, (1 << tag_bits) - 1) and 0 < serial < 2000
    t0 = on_device(owners)
    p.set_option("ec_tag_bits", tag_bits)
    try:
        eq.reset().add_rows(t0.data_ptr(), len(owners))
        assert eq.stats()[3] == 0
        for n in (1, 2):
            eq.add_rows(t.data_ptr(), len(rows))
            assert_all(eq, classes_of_rows(np.concatenate([owners] + [rows] * n), n_colors), n_colors, "W=%d, %d tag bits, the owners first, add %d" % (W, tag_bits, n),
                       n_rows=len(owners) + 2000 * n)
            assert eq.stats()[3] == serial * n
    finally:
        p.set_option("ec_tag_bits", None)
    eq.close(); col.close()


# ---- 5. capacity -----------------------------------------------------------------------------------------------------------------------
def test_capacity(small):
    p, g, rng = small
    n_colors = 128
    col = p.colors(n_colors)
    pool = np.unique(rng.integers(1, 1 << 63, size=(210, 2), dtype=np.uint64), axis=0)
    assert len(pool) == 210
    eq = col.eqclasses(100)
    hundred = pool[rng.integers(0, 100, 900)]
    hundred[:100] = pool[:100]
    t100, t1, t200 = on_device(hundred), on_device(pool[100:101]), on_device(pool[:200])
    eq.add_rows(t100.data_ptr(), len(hundred))
    assert_all(eq, classes_of_rows(hundred, n_colors), n_colors, "exactly max_classes distinct rows", n_rows=900)
    eq.add_rows(t1.data_ptr(), 1)              # one more class in a later add
    for _ in range(2):
        with pytest.raises(fa.FinitoError) as e:
            eq.download()
        assert e.value.code == fa.FIN_ELIMIT and "max_classes" in str(e.value)
    eq.reset().add_rows(t100.data_ptr(), len(hundred))
    assert_all(eq, classes_of_rows(hundred, n_colors), n_colors, "after the reset", n_rows=900)
    eq.close()
    eq = col.eqclasses(4)                      # 8 slots, 200 distinct rows: the probe bound ends every chain
    eq.add_rows(t200.data_ptr(), 200)
    with pytest.raises(fa.FinitoError) as e:
        eq.download()
    assert e.value.code == fa.FIN_ELIMIT
    four = pool[rng.integers(0, 4, 300)]
    t4 = on_device(four)
    eq.reset().add_rows(t4.data_ptr(), len(four))
    assert_all(eq, classes_of_rows(four, n_colors), n_colors, "a good add after the reset", n_rows=300)
    eq.close()
    for bad in (0, (1 << 26) + 1):
        with pytest.raises(fa.FinitoError) as e:
            col.eqclasses(bad)
        assert e.value.code == fa.FIN_ELIMIT
    col.close()


# ---- 6. across adds and streams --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def set31():
    rng = np.random.default_rng(22900)
    k = 31
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=700)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    reads = read_families(rng, g, k, unitigs, n=800)
    n_colors = 70
    bits, picked = hand_picked(unitigs, k, random_matrix(rng, len(unitigs), n_colors), n_colors)
    reads = reads + picked
    bits.setflags(write=False)
    yield p, o, g, unitigs, reads, bits, n_colors, rng
    p.close()


def test_adds_and_a_reset_on_several_streams(set31):
    p, o, g, unitigs, reads, bits, n_colors, rng = set31
    k = 31
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream(), None]
    parts = [reads[0:200], reads[200:450], reads[450:600], reads[600:]]
    col = p.colors(n_colors, bits)
    eq = col.eqclasses(4096)
    batches = []
    for part, s, mode in zip(parts, streams, (2, 0, 2, 0)):
        b = p.batch(part); b.text_mode(mode); b.run(fa.FIN_MERGED, stream=s.cuda_stream if s else None)
        batches.append(b)
    sid = lambda s: s.cuda_stream if s else None
    eq.add(batches[0], 1000, stream=sid(streams[1]))   # (on another stream than the run's)
    eq.add(batches[1], 1000, stream=sid(streams[0]))
    eq.reset(stream=sid(streams[2]))
    eq.add(batches[2], 1000, stream=sid(streams[3]))
    eq.add(batches[3], 1000, stream=sid(streams[2]))
    later = parts[2] + parts[3]
    want = classes_of_rows(rows_of(oracle_pairs(o, later), nks_of(later, k), bits, n_colors, 1000)[0], n_colors)
    assert_all(eq, want, n_colors, "the adds after the reset", n_rows=len(later))
    # the same classes from two streams, one add issued right behind the other: the second add's claims run behind the first add's rows
    rows = rows_of(oracle_pairs(o, parts[0]), nks_of(parts[0], k), bits, n_colors, 0)[0]
    t = on_device(rows)
    eq.reset()
    eq.add_rows(t.data_ptr(), len(rows), stream=sid(streams[0]))
    eq.add_rows(t.data_ptr(), len(rows), stream=sid(streams[1]))
    assert_all(eq, times(classes_of_rows(rows, n_colors), 2), n_colors, "two streams, the same classes", n_rows=2 * len(rows))
    for b in batches:
        b.close()
    eq.close(); col.close()


def test_host_buffers(set31):
    p, o, g, unitigs, reads, bits, n_colors, rng = set31
    k = 31
    nks = nks_of(reads, k)
    col = p.colors(n_colors, bits)
    eq = col.eqclasses()
    for strands in (fa.FIN_MERGED, fa.FIN_FWD):
        e = oracle_pairs(o, reads, strands)
        for pm in (1000, 300):
            want = classes_of_rows(rows_of(e, nks, bits, n_colors, pm)[0], n_colors)
            assert eq.reset().add_reads(reads, pm, strands) is eq
            assert_all(eq, want, n_colors, "host buffers, strands %d, permille %d" % (strands, pm), n_rows=len(reads))
    want = classes_of_rows(rows_of(oracle_pairs(o, reads), nks, bits, n_colors, 1000)[0], n_colors)
    p.set_option("max_batch_kmers", int(nks.sum()) // 6); p.set_option("pipeline_depth", 3)
    try:
        eq.reset().add_reads(reads)
    finally:
        p.set_option("max_batch_kmers", None); p.set_option("pipeline_depth", None)
    assert_all(eq, want, n_colors, "host buffers, six sub-batches", n_rows=len(reads))
    eq.add_reads([]).add_reads(["", "ACG", g[:30]])   # nothing, and reads shorter than k: unaligned rows
    assert_all(eq, (want[0], want[1], want[2] + 3), n_colors, "host buffers, reads without k-mers", n_rows=len(reads) + 3)
    eq.close(); col.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(set31):
    p, o, g, unitigs, reads, bits, n_colors, rng = set31
    col = p.colors(n_colors, bits)
    eq = col.eqclasses(1024)
    b = p.batch(reads[:50])
    with pytest.raises(fa.FinitoError) as e:       # a batch that has not run
        eq.add(b)
    assert e.value.code == fa.FIN_EINVAL
    b.run(fa.FIN_MERGED)
    with pytest.raises(fa.FinitoError) as e:
        eq.add(b, 1001)
    assert e.value.code == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:
        eq.add_reads(reads[:10], 1001)
    assert e.value.code == fa.FIN_EINVAL
    p2 = fa.FinimizerIndex.build(unitigs, 31).to_device(0)   # colours of another index
    foreign = p2.colors(n_colors)
    feq = foreign.eqclasses(16)
    with pytest.raises(fa.FinitoError) as e:
        feq.add(b)
    assert e.value.code == fa.FIN_EINVAL
    err = fa.C.create_string_buffer(512)
    bases, offsets = fa.flatten(reads[:10])
    assert fa.lib().fin_search_batch_add_eqclasses(p.h, bases.ctypes.data_as(fa.C.c_char_p), offsets.ctypes.data_as(fa.C.POINTER(fa.C.c_uint64)), 10, fa.FIN_MERGED, feq.h,
                                                   1000, err, 512) == fa.FIN_EINVAL and b"another index" in err.value
    assert feq.stats()[0] == 0 and eq.stats()[0] == 0
    feq.close(); foreign.close(); p2.close()
    with pytest.raises(fa.FinitoError) as e:       # no replica: no colours, so no accumulator
        fa.FinimizerIndex.build(unitigs[:5], 31).colors(5).eqclasses()
    assert e.value.code == fa.FIN_ENODEV
    eq.add(b)
    assert eq.stats()[0] == 50
    b.close(); eq.close(); col.close()


def test_a_withheld_run_adds_nothing():
    """tests/test_colors.py::test_a_withheld_step_colours_nothing_has_no_rows_and_is_reported_until_the_reset's recipe: a step whose overflow list overran has no
    rows, the add reports FIN_ELIMIT and adds nothing, and the accumulator goes on working"""
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    reads = sample_reads(rng, g, 500, 150)
    bits = random_matrix(rng, len(unitigs), 5)
    L = fa.lib()
    col = p.colors(5, bits)
    eq = col.eqclasses(64)
    try:
        good = p.batch(reads[:100]); good.text_mode(2); good.run(fa.FIN_MERGED)
        eq.add(good)
        before = eq.stats()
        assert before[0] == 100
        assert L.fin_set_option(b"lds_deque_limit", 1) == 0 and L.fin_set_option(b"seed_anchors", 0) == 0 and L.fin_set_option(b"debug_ovf_cap", 3) == 0
        for mode in (0, 2):
            b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
            with pytest.raises(fa.FinitoError) as e:
                eq.add(b)
            assert e.value.code == fa.FIN_ELIMIT and "overflow list" in str(e.value)
            assert eq.stats() == before
            b.close()
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        eq.reset().add(b)
        want = classes_of_rows(rows_of(oracle_pairs(o, reads), nks_of(reads, k), bits, 5, 1000)[0], 5)
        assert_all(eq, want, 5, "a good step afterwards", n_rows=len(reads))
        b.close(); good.close()
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)
        eq.close(); col.close(); p.close()
