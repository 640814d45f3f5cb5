"""Deduplicated colour sets on the device (fin_colors_compact and the compact state of fin_colors).  Every comparison is exact; the expectation is
numpy over the dense matrix (tests/test_colors_host.py::rows_of, np.unique), never a device output."""
import numpy as np
import pytest
import torch

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.test_colors import PERMILLES, hand_picked
from tests.test_colors_host import assert_pseudo, random_matrix, rows_of, words_of
from tests.test_colorsets_host import canonical_of
from tests.test_paired_host import assert_frags, frags_of
from tests.test_records_device import inject
from tests.test_segments import nks_of, oracle_pairs
from tests.test_unitig_counts import read_families
from tests.util import cut_unitigs, hand_made_case, random_genome

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


def ec_mix(x):
    x ^= x >> 30; x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27; x = x * 0x94D049BB133111EB & M64
    return x ^ (x >> 31)


def tag_and_home(row, tag_bits, slots):
    """fin_colorsets.hip's tag and home slot of a row, restated: the row's hash is fin_rowhash.h's"""
    h = 0
    for i, w in enumerate(row.tolist()):
        h ^= ec_mix((w + (i + 1) * 0x9E3779B97F4A7C15) & M64)
    tag = (h >> 33) & ((1 << tag_bits) - 1)
    return tag, ~(ec_mix(tag) >> 7) & (slots - 1)


def slots_of(max_sets):
    lg = 1
    while (1 << lg) < 2 * max_sets:
        lg += 1
    return 1 << lg


@pytest.fixture(scope="module")
def many():
    """an index of many short unitigs: several blocks of 256, the last wave and the last block not full"""
    k = 31
    rng = np.random.default_rng(3801)
    g = random_genome(rng, 40000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, k, max_len=80), k).to_device(0)
    assert p.n_unitigs >= 600 and p.n_unitigs % 64 != 0
    yield p, rng
    p.close()


def with_duplicates(rng, nu, n_colors):
    """a random matrix in which a few hundred rows are copies of others; one row also at 0, 1, 63 (one wave), 64 (the next), 255, 256 and 520 (other blocks)"""
    bits = random_matrix(rng, nu, n_colors)
    src = rng.integers(0, nu, 300)
    bits[rng.permutation(nu)[:300]] = bits[src]
    one = bits[bits.any(axis=1)][0]
    bits[[0, 1, 63, 64, 255, 256, 520]] = one
    return bits


def assert_invariant(col, bits, what):
    set_of, sets = col.download_sets()
    ne = bits[bits.any(axis=1)]
    n_distinct = len(np.unique(ne, axis=0)) if len(ne) else 0
    assert col.is_compact and col.n_sets == n_distinct == len(sets) - 1, what
    assert set_of.dtype == np.uint32 and sets.dtype == np.uint64 and set_of.shape == (len(bits),), what
    assert not sets[0].any() and sets[1:].any(axis=1).all() and len(np.unique(sets[1:], axis=0)) == n_distinct, what
    assert np.array_equal(sets[set_of], bits), what
    assert np.array_equal((set_of == 0), ~bits.any(axis=1)), what
    # canonicalised on the host, the device's sets are the twin's
    order = np.lexsort(sets[1:].T[::-1]) if n_distinct else np.zeros(0, dtype=np.int64)
    rank = np.zeros(n_distinct + 1, dtype=np.uint32); rank[order + 1] = np.arange(1, n_distinct + 1, dtype=np.uint32)
    t_of, t_sets = fa.unitig_color_sets(bits, col.n_colors)
    assert np.array_equal(sets[1:][order], t_sets[1:]) and np.array_equal(rank[set_of], t_of), what
    assert np.array_equal(t_of, canonical_of(bits)[0]) and np.array_equal(t_sets, canonical_of(bits)[1]), what
    return set_of, sets


@pytest.mark.parametrize("n_colors", [40, 100, 130, 4096])
def test_the_invariant_after_compact(many, n_colors):
    p, rng = many
    nu = p.n_unitigs
    bits = with_duplicates(rng, nu, n_colors)
    n_set = int(sum(bin(w).count("1") for w in bits.reshape(-1).tolist()))
    col = p.colors(n_colors, bits)
    dense_ptr = col.device_ptr()
    assert dense_ptr and not col.is_compact and col.n_sets == 0 and col.device_sets_ptr() == 0 and col.device_set_of_ptr() == 0 and col.compact_stats() == (0, 0, 0, 0)
    with pytest.raises(fa.FinitoError) as e:
        col.download_sets()
    assert e.value.code == fa.FIN_EINVAL
    assert col.expand() is col and col.device_ptr() == dense_ptr          # a no-op on a dense object
    col.compact()
    what = "%d colours" % n_colors
    set_of, sets = assert_invariant(col, bits, what)
    assert col.device_ptr() == 0 and col.device_sets_ptr() and col.device_set_of_ptr(), what
    st = col.compact_stats()
    assert st[0] == col.n_sets and st[3] == slots_of(nu), what
    got, got_set = col.download()
    assert np.array_equal(got, bits) and got_set == n_set and col.is_compact, what
    ptrs = (col.device_sets_ptr(), col.device_set_of_ptr())
    col.compact()                                                         # twice: a no-op
    assert (col.device_sets_ptr(), col.device_set_of_ptr()) == ptrs and col.compact_stats() == st
    s2 = col.download_sets()
    assert np.array_equal(s2[0], set_of) and np.array_equal(s2[1], sets)
    col.expand()
    assert col.device_ptr() and not col.is_compact and col.n_sets == 0 and col.device_sets_ptr() == 0
    got, got_set = col.download()
    assert np.array_equal(got, bits) and got_set == n_set, what
    # upload and reset leave a compact object dense
    col.compact(); col.upload(bits[::-1].copy())
    assert not col.is_compact and np.array_equal(col.download()[0], bits[::-1])
    col.compact(); col.reset()
    assert not col.is_compact and col.device_ptr() and col.download()[1] == 0
    col.compact()                                                         # all rows empty: no set but the empty one
    assert col.n_sets == 0 and not col.download_sets()[0].any() and col.download()[1] == 0
    col.close()


def test_where_the_table_can_go_wrong(many):
    p, rng = many
    nu = p.n_unitigs
    n_colors = 130
    bits = with_duplicates(rng, nu, n_colors)
    bits[:500, 0] = (bits[:500, 0] & ~np.uint64(0x3FF)) | np.arange(1, 501, dtype=np.uint64)      # 500 rows that are certainly distinct, then copies of them
    bits[rng.permutation(np.arange(500, nu))[:300]] = bits[rng.integers(0, 500, 300)]
    bits[[520, 777, nu - 1]] = bits[0]; bits[[1, 63, 64, 255, 256]] = bits[0]; bits[2:63] = bits[2]; bits[65:255] = bits[65]; bits[257:500] = bits[257]
    distinct = np.unique(bits[bits.any(axis=1)], axis=0)
    nd = len(distinct)
    assert nd >= 450
    col = p.colors(n_colors, bits)
    try:
        # narrow tags: distinct rows under one tag are told apart by the row compare
        for tb in (1, 2):
            p.set_option("colorsets_tag_bits", tb)
            col.compact()
            assert_invariant(col, bits, "tag bits %d" % tb)
            st = col.compact_stats()
            assert st[0] == nd and st[1] > 0 and st[2] >= nd // (1 << tb) - 1 and st[3] == slots_of(nu), st
            col.expand()
        # max_sets: the distinct count exactly passes, one fewer is FIN_ELIMIT and the object stays dense with its matrix intact
        p.set_option("colorsets_tag_bits", None)
        for tb in (None, 1):
            p.set_option("colorsets_tag_bits", tb)
            ptr = col.device_ptr()
            with pytest.raises(fa.FinitoError) as e:
                col.compact(max_sets=nd - 1)
            assert e.value.code == fa.FIN_ELIMIT and not col.is_compact and col.device_ptr() == ptr and col.n_sets == 0
            assert np.array_equal(col.download()[0], bits)
            col.compact(max_sets=nd)
            assert_invariant(col, bits, "max_sets = the distinct rows, tag bits %s" % tb)
            assert col.compact_stats()[3] == slots_of(nd)
            col.expand()
        with pytest.raises(fa.FinitoError) as e:
            col.compact(max_sets=(1 << 26) + 1)
        assert e.value.code == fa.FIN_ELIMIT and not col.is_compact
        # probes that wrap past the last slot: tag 0's home is the last slot, its n_0 distinct rows need a slot each, so all but one of them went round the
        # end and the farthest lies at least n_0 - 1 slots behind its home -- more than the distance from that home to the table's end, which is 0
        for tb, max_sets in ((1, nd), (2, nd), (3, 3 * nd)):
            slots = slots_of(max_sets)
            th = [tag_and_home(r, tb, slots) for r in distinct]
            n_0 = sum(1 for t, h in th if t == 0)
            assert n_0 >= 20 and all(h == slots - 1 for t, h in th if t == 0) and ec_mix(0) == 0
            p.set_option("colorsets_tag_bits", tb)
            col.compact(max_sets=max_sets)
            assert_invariant(col, bits, "a wrapping probe: tag bits %d, %d slots" % (tb, slots))
            st = col.compact_stats()
            assert st[3] == slots and st[2] >= n_0 - 1 > slots - 1 - (slots - 1) and st[1] > 0, (st, n_0)
            col.expand()
    finally:
        p.set_option("colorsets_tag_bits", None)
    col.close()


def test_a_flagged_matrix_is_not_compacted():
    """the recipe of tests/test_colors.py::test_a_withheld_step_colours_nothing_has_no_rows_and_is_reported_until_the_reset"""
    from tests.util import sample_reads
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, k, max_len=500), k).to_device(0)
    reads = sample_reads(rng, g, 500, 150)
    L = fa.lib()
    col = p.colors(5)
    try:
        assert L.fin_set_option(b"lds_deque_limit", 1) == 0 and L.fin_set_option(b"seed_anchors", 0) == 0 and L.fin_set_option(b"debug_ovf_cap", 3) == 0
        b = p.batch(reads); b.text_mode(0); b.run(fa.FIN_MERGED)
        col.add(b, 3)
        with pytest.raises(fa.FinitoError) as e:
            col.compact()
        assert e.value.code == fa.FIN_ELIMIT and "overflow list" in str(e.value) and not col.is_compact and col.device_ptr()
        col.reset().compact()
        assert col.is_compact and col.n_sets == 0
        b.close()
    finally:
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0 and L.fin_set_option(b"lds_deque_limit", 16) == 0 and L.fin_set_option(b"seed_anchors", 1) == 0
    col.close(); p.close()


def pair_reads(reads):
    return reads if len(reads) % 2 == 0 else reads[:-1]


@pytest.mark.parametrize("k", [16, 31, 127])
def test_pseudoalignment_parity(k):
    """the compact state against numpy over the dense matrix: every read family, text modes 0, 1 and 2, per read and per fragment"""
    rng = np.random.default_rng(3800 + k)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=max(700, 4 * k))
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    fam = read_families(rng, g, k, unitigs, n=400)
    mats, reads = {}, None
    for n_colors in (5, 65, 130):
        mats[n_colors], picked = hand_picked(unitigs, k, random_matrix(rng, len(unitigs), n_colors), n_colors)
        reads = pair_reads(fam + picked)
    nks = nks_of(reads, k)
    e1 = oracle_pairs(o, reads)
    cols = {n: p.colors(n, mats[n]).compact() for n in mats}
    for n in mats:
        assert_invariant(cols[n], mats[n], "k=%d, %d colours" % (k, n))
    want = {n: {pm: rows_of(e1, nks, mats[n], n, pm) for pm in PERMILLES} for n in mats}
    wantf = {n: {pm: frags_of(e1, nks, mats[n], n, pm) for pm in PERMILLES} for n in mats}
    for mode in (0, 1, 2):
        b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        for n in mats:
            for pm in PERMILLES:
                what = "k=%d text mode %d, %d colours, permille %d" % (k, mode, n, pm)
                assert_pseudo(b.pseudoalign(cols[n], pm), want[n][pm], what)
                assert_frags(b.pseudoalign_pairs(cols[n], pm), wantf[n][pm], what)
                assert_frags(b.pseudoalign_pairs(cols[n], pm, both=True), frags_of(e1, nks, mats[n], n, pm, both=True), what + ", both")
        if k <= 63 and mode:
            assert b.pipeline_counts()[41] > 0      # the record path was really taken
        b.close()
    for c in cols.values():
        c.close()
    p.close()


def test_parity_at_4096_colours():
    k = 31
    rng = np.random.default_rng(3896)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=700)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    bits, picked = hand_picked(unitigs, k, random_matrix(rng, len(unitigs), 4096), 4096)
    rd = pair_reads(read_families(rng, g, k, unitigs, n=150) + picked)
    e1, nk = oracle_pairs(o, rd), nks_of(rd, k)
    col = p.colors(4096, bits).compact()
    for mode in (0, 2):
        b = p.batch(rd); b.text_mode(mode); b.run(fa.FIN_MERGED)
        for pm in PERMILLES:
            assert_pseudo(b.pseudoalign(col, pm), rows_of(e1, nk, bits, 4096, pm), "4096 colours, mode %d, permille %d" % (mode, pm))
            assert_frags(b.pseudoalign_pairs(col, pm), frags_of(e1, nk, bits, 4096, pm), "4096 colours, fragments, mode %d, permille %d" % (mode, pm))
        b.close()
    col.close(); p.close()


@pytest.mark.parametrize("n_colors", [40, 130])
def test_the_two_sides_of_the_64_entry_table(many, n_colors):
    """hand-made pairs (set_pairs, text mode 0: every read is scanned).  The table is keyed by set id: a read of 200 unitigs that carry 3 (or 64) sets stays on it,
    a read of more than 64 sets is rescanned; both exact.  All unitigs of set 0; unitig numbers at or above n_unitigs"""
    p, rng = many
    k, nu = 31, p.n_unitigs
    A = (-1, -1)
    # 100 sets (one of them empty) dealt to the unitigs, so that a read's distinct unitigs and distinct sets can be chosen apart
    pool = random_matrix(rng, 800, n_colors)
    pool = np.unique(pool[pool.any(axis=1)], axis=0)[:99]
    assert len(pool) == 99
    which = np.where(rng.random(nu) < 0.3, rng.integers(0, 3, nu), rng.integers(3, 100, nu))        # 99: the empty row; sets 0, 1 and 2 are common
    bits = np.concatenate([pool, np.zeros((1, pool.shape[1]), np.uint64)])[which]
    of_set = lambda s, n: [int(u) for u in np.nonzero(which == s)[0][:n]]
    cases = {
        "200 unitigs of 3 sets": [(u, i) for s in (0, 1, 2) for u in of_set(s, 5) for i in range(2)] * 1 + [(int(u), 0) for u in np.nonzero(which < 3)[0]],
        "many unitigs of exactly 64 sets": [(int(u), 0) for u in np.nonzero(which < 64)[0]],
        "65 sets": [(int(u), 0) for u in np.nonzero(which < 65)[0]],
        "every set": [(int(u), i) for u in rng.permutation(nu)[:600] for i in range(2)],
        "unitigs of set 0 only": [(int(u), 0) for u in np.nonzero(which == 99)[0]] + [A] * 3,
        "outside the index": [(nu, 0), (nu + 5, 1), (0x7FFFFFFF, 0), (-2, 0), (3, 1), A, (4, 0)],
        "outside the index among 70 sets": [(int(u), 0) for u in np.nonzero(which < 70)[0][:150]] + [(nu, 0), (nu + 1, 0)] * 5,
        "nothing": [A] * 70,
        "empty": [],
    }
    names = list(cases)
    distinct_u = lambda c: len({u for u, _ in c if 0 <= u < nu})
    distinct_s = lambda c: len({int(which[u]) for u, _ in c if 0 <= u < nu and which[u] != 99})
    assert distinct_u(cases["200 unitigs of 3 sets"]) > 200 and distinct_s(cases["200 unitigs of 3 sets"]) == 3
    assert distinct_u(cases["many unitigs of exactly 64 sets"]) > 64 and distinct_s(cases["many unitigs of exactly 64 sets"]) == 64
    assert distinct_s(cases["65 sets"]) == 65 and distinct_s(cases["every set"]) > 80 and distinct_u(cases["unitigs of set 0 only"]) > 0
    if len(names) % 2:
        names.append("empty")
    pairs = np.array([x for n in names for x in cases[n]], dtype=np.int32).reshape(-1, 2)
    nks = np.array([len(cases[n]) for n in names])
    reads = [random_genome(rng, int(nk) + k - 1) if nk else "ACGT" for nk in nks]
    b = p.batch(reads); b.text_mode(0); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(pairs)
    dense = p.colors(n_colors, bits)
    col = p.colors(n_colors, bits).compact()
    assert col.n_sets == 99
    b.pseudoalign(col)
    b.set_pairs(pairs)
    for pm in (0, 300, 500, 1000):
        want = rows_of(pairs, nks, bits, n_colors, pm)
        rows, heads = b.pseudoalign(col, pm)
        for i, n in enumerate(names):
            assert tuple(heads[i].tolist()) == tuple(want[1][i].tolist()) and np.array_equal(rows[i], want[0][i]), \
                "%s, %d colours, permille %d: got %s %s, want %s %s" % (n, n_colors, pm, heads[i], rows[i], want[1][i], want[0][i])
        assert_pseudo(b.pseudoalign(dense, pm), want, "the dense matrix, permille %d" % pm)
        for both in (False, True):
            wantf = frags_of(pairs, nks, bits, n_colors, pm, both)
            assert_frags(b.pseudoalign_pairs(col, pm, both), wantf, "fragments, %d colours, permille %d, both %s" % (n_colors, pm, both))
            assert_frags(b.pseudoalign_pairs(dense, pm, both), wantf, "fragments over the dense matrix, permille %d" % pm)
    b.close(); col.close(); dense.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_hand_made_records_over_sets(mode):
    """the kind-1 branch: a record's unitig becomes its set id; W = 1 and W = 2"""
    k = 16
    c = hand_made_case(k)
    rng = np.random.default_rng(3850)
    p = fa.FinimizerIndex.build(c.unitigs, k).to_device(0)
    b = p.batch(c.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
    inject(b, c.recs, c.pairs, mode)
    for n_colors in (1, 65):
        bits = random_matrix(rng, len(c.unitigs), n_colors)
        bits[rng.permutation(len(bits))[: len(bits) // 2]] = bits[0]
        col = p.colors(n_colors, bits).compact()
        for pm in PERMILLES:
            assert_pseudo(b.pseudoalign(col, pm), rows_of(c.pairs, c.nks, bits, n_colors, pm), "text mode %d, %d colours, permille %d" % (mode, n_colors, pm))
            if len(c.nks) % 2 == 0:
                assert_frags(b.pseudoalign_pairs(col, pm), frags_of(c.pairs, c.nks, bits, n_colors, pm), "fragments, text mode %d, %d colours" % (mode, n_colors))
        col.close()
    b.close(); p.close()


@pytest.fixture(scope="module")
def set31():
    rng = np.random.default_rng(3831)
    k = 31
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=700)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    reads = pair_reads(read_families(rng, g, k, unitigs, n=400))
    yield p, unitigs, reads, rng
    p.close()


def test_downstream_is_bit_identical(set31):
    p, unitigs, reads, rng = set31
    n_colors = 70
    bits = random_matrix(rng, len(unitigs), n_colors)
    dense, col = p.colors(n_colors, bits), p.colors(n_colors, bits).compact()
    b = p.batch(reads); b.text_mode(1); b.run(fa.FIN_MERGED)
    out = {}
    for name, c in (("dense", dense), ("compact", col)):
        eq = c.eqclasses(1 << 12)
        eq.add(b, 300); eq.add_pairs(b, 1000)
        rows, n_reads, unaligned = eq.download()
        ab = eq.abundance()
        asg = c.assigner(ab.weights(), 0.3)
        asg.add(b, 300); asg.add(b, 1000, pairs=True)
        out[name] = (rows, n_reads, unaligned, ab.alpha, ab.iters) + tuple(asg.download())
        asg.close(); eq.close()
    assert len(out["dense"][0]) > 10 and out["dense"][3].sum() > 0
    for x, y in zip(out["dense"], out["compact"]):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    assert out["dense"][3].tobytes() == out["compact"][3].tobytes()     # alpha bit for bit
    # what writes or reads bits[u * W + w] wants the dense matrix
    cover = p.cover()
    for call in (lambda: col.add(b, 3), lambda: col.add_reads(reads[:10], 3), lambda: col.coverage(), lambda: col.coverage(cover), lambda: col.shared(),
                 lambda: col.taxonomy(np.zeros(3, np.uint32), np.ones(n_colors, np.uint32))):
        with pytest.raises(fa.FinitoError) as e:
            call()
        assert e.value.code == fa.FIN_EINVAL and "fin_colors_expand" in str(e.value), str(e.value)
    assert col.is_compact and np.array_equal(col.download()[0], bits)
    col.expand()
    col.add(b, 3); col.coverage(); col.shared(); col.taxonomy(np.zeros(3, np.uint32), np.ones(n_colors, np.uint32)).close()
    cover.close(); b.close(); col.close(); dense.close()


def test_upload_sets(set31):
    p, unitigs, reads, rng = set31
    n_colors, nu = 70, len(unitigs)
    bits = random_matrix(rng, nu, n_colors)
    bits[rng.permutation(nu)[: nu // 2]] = bits[1]
    set_of, sets = fa.unitig_color_sets(bits, n_colors)
    ns = len(sets) - 1
    b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
    ref = p.colors(n_colors, bits)
    want = {pm: b.pseudoalign(ref, pm) for pm in PERMILLES}
    col = p.colors(n_colors, set_of=set_of, sets=sets)
    assert col.is_compact and col.n_sets == ns and col.device_ptr() == 0 and np.array_equal(col.download()[0], bits)
    # duplicates and unused sets: every set twice, the even unitigs use the copy; two sets that nobody uses
    more = np.concatenate([sets, sets[1:], np.full((2, sets.shape[1]), 3, dtype=np.uint64)])
    moved = np.where((np.arange(nu) % 2 == 0) & (set_of > 0), set_of + ns, set_of).astype(np.uint32)
    col2 = p.colors(n_colors, bits).compact().upload_sets(moved, more)     # over a compact object
    assert col2.n_sets == 2 * ns + 2 and np.array_equal(col2.download()[0], bits) and col2.download()[1] == ref.download()[1]
    got_of, got_sets = col2.download_sets()
    assert np.array_equal(got_of, moved) and np.array_equal(got_sets, more)
    for c in (col, col2):
        for pm in PERMILLES:
            assert_pseudo(b.pseudoalign(c, pm), want[pm], "uploaded sets, permille %d" % pm)
    assert_pseudo(want[1000], rows_of(oracle_pairs(OracleIndex.build(unitigs, 31), reads), nks_of(reads, 31), bits, n_colors, 1000), "the dense reference")
    col2.expand()
    assert np.array_equal(col2.download()[0], bits)
    # each refused input, named; the object is unchanged
    bad_of = np.array(set_of); bad_of[7] = ns + 1
    bad0 = np.array(sets); bad0[0, 1] = 1
    stray = np.array(sets); stray[3, 1] |= np.uint64(1) << np.uint64(6)     # colour 70 of 70
    for so, st, word in ((bad_of, sets, "unitig 7"), (set_of, bad0, "set 0"), (set_of, stray, "set 3")):
        with pytest.raises(fa.FinitoError) as e:
            col.upload_sets(so, st)
        assert e.value.code == fa.FIN_EINVAL and word in str(e.value), str(e.value)
    for so, st in ((set_of[:-1], sets), (set_of, sets[:, :1]), (set_of, None)):
        with pytest.raises(fa.FinitoError):
            col.upload_sets(so, st) if st is not None else p.colors(n_colors, set_of=so)
    assert col.is_compact and np.array_equal(col.download()[0], bits)
    b.close(); col.close(); col2.close(); ref.close()


def test_compact_and_expand_on_a_stream(set31):
    """compact and expand on a non-default stream behind an add on another one, then a pseudoalignment on the batch's stream (tests/test_streams.py's style)"""
    from tests.test_streams import Delay
    p, unitigs, reads, rng = set31
    n_colors = 70
    S, T, U = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    delay = Delay()
    bits = random_matrix(rng, len(unitigs), n_colors)
    o = OracleIndex.build(unitigs, 31)
    e1, nks = oracle_pairs(o, reads), nks_of(reads, 31)
    met = np.unique(e1[e1[:, 0] >= 0, 0])
    want_bits = np.array(bits); want_bits[met, 0] |= np.uint64(1) << np.uint64(2)
    col = p.colors(n_colors, bits)
    b = p.batch(reads); b.text_mode(1)
    b.run(fa.FIN_MERGED, stream=S.cuda_stream)
    delay(T, 50)
    col.add(b, 2, stream=T.cuda_stream)                # behind the delay on T
    col.compact(stream=U.cuda_stream)                  # on U: behind the add on T
    assert_invariant(col, want_bits, "compact on a stream behind an add on another")
    for pm in PERMILLES:
        assert_pseudo(b.pseudoalign(col, pm), rows_of(e1, nks, want_bits, n_colors, pm), "after compact on a stream, permille %d" % pm)
    col.expand(stream=T.cuda_stream)
    col.add(b, 5, stream=U.cuda_stream)                # behind the expand on T
    want_bits[met, 0] |= np.uint64(1) << np.uint64(5)
    assert_pseudo(b.pseudoalign(col, 1000), rows_of(e1, nks, want_bits, n_colors, 1000), "after expand on a stream")
    assert np.array_equal(col.download()[0], want_bits)
    torch.cuda.synchronize()
    b.close(); col.close()
