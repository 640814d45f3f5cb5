"""Paired-end pseudoalignment on the device (include/finito_amd.h: fin_batch_pseudoalign_paired, fin_batch_add_eqclasses_paired, fin_search_batch_*_paired;
fin_paired.hip).  The expectation is always the numpy definition -- tests/test_colors_host.py::rows_of over the ORACLE's pairs, or over hand-made
pairs, with a fragment's slots its mates' slots back to back (tests/test_paired_host.py::frags_of) --, never a device output or a fin_records_* result; every
comparison is exact."""
import numpy as np
import pytest
import torch

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.test_abundance_host import Model, assert_one_iteration, rtol1
from tests.test_colors_host import assert_pseudo, pack, random_matrix, rows_of
from tests.test_eqclasses_host import assert_classes, classes_of_rows
from tests.test_paired_host import PERMILLES, assert_frags, frags_of, only_both
from tests.test_read_class import numbers_of
from tests.test_records_device import inject
from tests.test_segments import nks_of, oracle_pairs
from tests.test_streams import Delay
from tests.test_unitig_counts import read_families
from tests.util import cut_unitigs, random_genome, rc

pytestmark = pytest.mark.gpu

COLORS = (5, 64, 65, 130)


def picked(unitigs, k, bits, n_colors):
    """four unitigs given rows of their own -- a {0}, b {last colour}, c {0 and the last colour}, d {} -- and the fragments made of them, mates first and second:
    disjoint sets (an empty AND of two non-empty rows); 60 k-mers of a and 20 of b (shares 750 and 250: permille 300 differs from 0 and from 1000); a coloured and
    an uncoloured mate (FIN_PAIR_BOTH zeroes what FIN_PAIR_ANY gives), either way round; overlapping sets; a mate shorter than k"""
    num = numbers_of(unitigs, k)
    a, b, c, d = [i for i in range(len(unitigs)) if len(unitigs[i]) >= k + 60][:4]
    bits = np.array(bits)
    top = n_colors - 1
    for i, cs in ((a, [0]), (b, [top]), (c, [0, top]), (d, [])):
        bits[num[i]] = pack([cs], n_colors)[0]
    A, B, Cc, D = (unitigs[i] for i in (a, b, c, d))
    return bits, [A[:k + 40], rc(B[:k + 40]), A[:k + 59], B[:k + 19], A[:k + 30], D[:k + 30], D[:k + 30], B[:k + 30], A[:k + 30], Cc[5:k + 50], Cc[:k + 9], "ACG"]


def fragments(rng, g, k, unitigs):
    """about 800 reads of every family shuffled into fragments, and fragments whose mates are exact pieces of ONE unitig, a piece and its reverse complement, a
    piece and a read without k-mers: interleaved, an even number"""
    fam = read_families(rng, g, k, unitigs, n=800)
    if len(fam) % 2:
        fam.append(fam[0])
    long = [u for u in unitigs if len(u) >= k + 30]
    for u in long[:24]:
        fam += [u[:k + 12], u[8:k + 30]]
    for u in long[24:32]:
        fam += [u[:k + 20], rc(u[:k + 20])]
    for u in long[32:36]:
        fam += [u[2:k + 20], g[10:10 + k - 1], "", u[:k + 5]]
    return fam


class World:
    def __init__(self, k):
        self.k = k
        rng = self.rng = np.random.default_rng(2700 + k)
        g = random_genome(rng, 40000)
        self.unitigs = cut_unitigs(rng, g, k, max_len=max(700, 4 * k))
        self.p = fa.FinimizerIndex.build(self.unitigs, k).to_device(0)
        self.o = OracleIndex.build(self.unitigs, k)
        base = fragments(rng, g, k, self.unitigs)
        self.mats = {}
        for n in COLORS:
            self.mats[n], extra = picked(self.unitigs, k, random_matrix(rng, len(self.unitigs), n), n)
        self.reads = base + extra
        assert len(self.reads) % 2 == 0
        self.nks = nks_of(self.reads, k)
        self.pairs = oracle_pairs(self.o, self.reads)
        for a in (self.nks, self.pairs):
            a.setflags(write=False)
        self.want = {n: {pm: frags_of(self.pairs, self.nks, self.mats[n], n, pm) for pm in PERMILLES} for n in COLORS}
        self.cols = {n: self.p.colors(n, self.mats[n]) for n in COLORS}

    def close(self):
        for c in self.cols.values():
            c.close()
        self.p.close()


@pytest.fixture(scope="module", params=[31, 127], ids=lambda k: "k%d" % k)
def w(request):
    world = World(request.param)
    yield world
    world.close()


def assert_expectation_shows_everything(w, n_colors):
    """the guards: what the fragments must show for the comparison to mean something, asserted on the expectation"""
    want = w.want[n_colors]
    per_read = rows_of(w.pairs, w.nks, w.mats[n_colors], n_colors, 1000)
    ra, rb = per_read[0][0::2], per_read[0][1::2]
    h = want[1000][1]
    two = (h["n_colored_first"] > 0) & (h["n_colored_first"] < h["n_colored"])
    assert two.any(), "no fragment with 0 < n_colored_first < n_colored"
    if n_colors > 1:
        assert (ra.any(axis=1) & rb.any(axis=1) & ~(ra & rb).any(axis=1)).any(), "no fragment whose AND is empty while both mates' rows are not"
        differ = (want[300][0] != want[0][0]).any(axis=1) & (want[300][0] != want[1000][0]).any(axis=1)
        assert differ.any(), "no fragment where 300 differs from 0 and from 1000"
    assert (~two & want[1000][0].any(axis=1)).any(), "no fragment where FIN_PAIR_BOTH zeroes a row that FIN_PAIR_ANY gives"
    # the identities, as a cross-check of the expectation itself: the AND or the other mate's row at 1000, the OR at 0
    ca, cb = per_read[1]["n_colored"][0::2], per_read[1]["n_colored"][1::2]
    assert np.array_equal(want[1000][0], np.where(((ca > 0) & (cb > 0))[:, None], ra & rb, np.where((ca > 0)[:, None], ra, rb)))
    at0 = rows_of(w.pairs, w.nks, w.mats[n_colors], n_colors, 0)[0]
    assert np.array_equal(want[0][0], at0[0::2] | at0[1::2])


def assert_every_kind_combination(recs):
    """on the records the step left (a guard on the input, not an expectation): (1,1) in one unitig and in two, (1,0), (0,1), (0,0), (1,2), (2,2), a mate
    shorter than k"""
    ka, kb = (recs["meta"][0::2] >> 16).astype(np.int64), (recs["meta"][1::2] >> 16).astype(np.int64)
    ua, ub, na, nb = recs["u"][0::2], recs["u"][1::2], recs["nk"][0::2], recs["nk"][1::2]
    both1 = (ka == 1) & (kb == 1)
    seen = {"(1,1) same unitig": (both1 & (ua == ub)).any(), "(1,1) different unitigs": (both1 & (ua != ub)).any(), "(1,0)": ((ka == 1) & (kb == 0) & (nb > 0)).any(),
            "(0,1)": ((ka == 0) & (na > 0) & (kb == 1)).any(), "(0,0)": ((ka == 0) & (kb == 0) & (na > 0) & (nb > 0)).any(),
            "(1,2) or (2,1)": (((ka == 1) & (kb == 2)) | ((ka == 2) & (kb == 1))).any(), "(2,2)": ((ka == 2) & (kb == 2)).any(), "a mate shorter than k": ((na == 0) | (nb == 0)).any()}
    assert all(seen.values()), "kind combinations that do not occur: %s" % [x for x in seen if not seen[x]]


def test_fragments_of_every_read_family_in_every_text_mode(w):
    """text modes 0, 1 and 2 under 5, 64, 65 and 130 colours, permille 0, 300 and 1000, both modes.  k = 127 leaves no records: every mate is scanned.  The per-read
    rows and the fragments' rows live side by side: each is bit-identical before and after the other call"""
    k, p = w.k, w.p
    for n in COLORS:
        assert_expectation_shows_everything(w, n)
    for mode in (0, 1, 2):
        b = p.batch(w.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        assert b.device_pair_ptrs() == (0, 0)
        for n in COLORS:
            for pm in PERMILLES:
                what = "k=%d text mode %d, %d colours, permille %d" % (k, mode, n, pm)
                assert_frags(b.pseudoalign_pairs(w.cols[n], pm), w.want[n][pm], what)
                assert_frags(b.pseudoalign_pairs(w.cols[n], pm, both=True), only_both(w.want[n][pm]), what + ", both")
        assert all(b.device_pair_ptrs())
        info = b.run_info()
        if k <= 63:
            assert info["fast_path"] and (mode == 0 or b.pipeline_counts()[41] > 0)
            if mode:
                assert_every_kind_combination(b.records()[0])
        else:
            assert not info["fast_path"] and b.pipeline_counts()[41] == 0
        # neither call touches the other's results
        frag = b.pseudoalign_pairs(w.cols[130], 300)
        assert b.device_pseudo_ptrs() == (0, 0)
        per_read = b.pseudoalign(w.cols[65], 1000)
        assert_pseudo(per_read, rows_of(w.pairs, w.nks, w.mats[65], 65, 1000), "k=%d text mode %d, per read" % (k, mode))
        L, err = fa.lib(), fa.C.create_string_buffer(512)
        rows, heads = np.zeros_like(frag[0]), np.zeros_like(frag[1])
        fa._check(L.fin_batch_download_pair_pseudo(b.h, rows.ctypes.data_as(fa.C.POINTER(fa.C.c_uint64)), heads.ctypes.data_as(fa.C.c_void_p), err, 512), err)
        assert rows.tobytes() == frag[0].tobytes() and heads.tobytes() == frag[1].tobytes(), "the fragments' rows changed under the per-read call"
        assert_frags(b.pseudoalign_pairs(w.cols[5], 0, both=True), only_both(w.want[5][0]), "k=%d text mode %d, after the per-read call" % (k, mode))
        rows, heads = np.zeros_like(per_read[0]), np.zeros_like(per_read[1])
        fa._check(L.fin_batch_download_pseudo(b.h, rows.ctypes.data_as(fa.C.POINTER(fa.C.c_uint64)), heads.ctypes.data_as(fa.C.c_void_p), err, 512), err)
        assert rows.tobytes() == per_read[0].tobytes() and heads.tobytes() == per_read[1].tobytes(), "the per-read rows changed under the paired call"
        # what forgets the per-read rows forgets the fragments' too; an odd number of reads is refused
        b.reload(w.reads[:51])
        assert b.device_pair_ptrs() == (0, 0)
        b.run(fa.FIN_MERGED)
        with pytest.raises(fa.FinitoError) as e:
            b.pseudoalign_pairs(w.cols[5])
        assert e.value.code == fa.FIN_EINVAL and "odd" in str(e.value) and b.device_pair_ptrs() == (0, 0)
        b.close()


def test_a_matrix_of_4096_colours(w):
    n_colors = 4096
    bits, extra = picked(w.unitigs, w.k, random_matrix(w.rng, len(w.unitigs), n_colors), n_colors)
    rd = w.reads[:200] + extra
    e1, nk = oracle_pairs(w.o, rd), nks_of(rd, w.k)
    col = w.p.colors(n_colors, bits)
    assert col.words == 64
    b = w.p.batch(rd); b.text_mode(2); b.run(fa.FIN_MERGED)
    for pm in PERMILLES:
        want = frags_of(e1, nk, bits, n_colors, pm)
        if pm == 0:
            assert (want[0][:, -1] >> np.uint64(63)).any() and (want[1]["n_colors"] > 64).any()
        assert_frags(b.pseudoalign_pairs(col, pm), want, "4096 colours, permille %d" % pm)
        assert_frags(b.pseudoalign_pairs(col, pm, both=True), only_both(want), "4096 colours, permille %d, both" % pm)
    b.close(); col.close()


# ---- hand-made records and pairs ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    """an index of more than 200 unitigs for hand-made records and pairs"""
    k = 31
    rng = np.random.default_rng(2764)
    g = random_genome(rng, 12000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, k, max_len=80), k).to_device(0)
    assert p.n_unitigs >= 200
    yield p, rng
    p.close()


def scan(slots):
    return ("scan", [(int(u), int(o)) for u, o in slots])


def rec1(u, n):
    """a kind-1 record: n found slots in unitig u"""
    return ("rec", int(u), int(n))


def walk(rng, us, absent=0.1):
    out = []
    for u in us:
        out += [(int(u), i) for i in range(int(rng.integers(1, 4)))]
        if rng.random() < absent:
            out.append((-1, -1))
    return out


def hand_made_fragments(rng, nu):
    """name -> (first mate, second mate)"""
    A = (-1, -1)
    perm = [int(u) for u in rng.permutation(nu)]
    f = {}
    f["40 + 40 distinct unitigs"] = (scan(walk(rng, perm[:40])), scan(walk(rng, perm[40:80])))
    f["40 + 40 unitigs, 20 shared: 60 fit"] = (scan(walk(rng, perm[:40])), scan(walk(rng, perm[20:60])))
    f["63 scanned + a new seed first: 64 fit"] = (rec1(perm[100], 7), scan(walk(rng, perm[:63])))
    f["63 scanned + a new seed second: 64 fit"] = (scan(walk(rng, perm[:63])), rec1(perm[100], 9))
    f["64 scanned + a new seed first: 65 overflow"] = (rec1(perm[100], 7), scan(walk(rng, perm[:64])))
    f["64 scanned + a new seed second: 65 overflow"] = (scan(walk(rng, perm[:64])), rec1(perm[100], 5))
    f["64 scanned + a seed among them: 64 fit"] = (rec1(perm[10], 6), scan(walk(rng, perm[:64])))
    f["the seed's unitig in the scanned mate"] = (rec1(perm[3], 11), scan([(perm[3], 0), (perm[4], 0), A, (perm[3], 5), (perm[5], 1)]))
    f["the seed's unitig in the scanned mate, seed second"] = (scan([(perm[3], 0), (perm[4], 0), A, (perm[3], 5), (perm[5], 1)]), rec1(perm[3], 2))
    f["a 130-slot mate and a seed"] = (scan([(perm[i % 3], i) for i in range(130)]), rec1(perm[1], 20))
    f["a 130-slot mate of 130 unitigs and a short mate"] = (scan([(perm[i], 0) for i in range(130)]), scan([(perm[7], 0), (perm[150], 0)]))
    f["two 70-slot mates over the same 70 unitigs"] = (scan([(perm[i], 0) for i in range(70)]), scan([(perm[69 - i], 1) for i in range(70)]))
    f["unitigs outside the index"] = (scan([(nu, 0), (nu + 5, 1), (0x7FFFFFFF, 0), (-2, 0), (perm[3], 1)]), scan([(perm[9], 0), (nu, 3)]))
    f["a record outside the index and a scanned mate"] = (rec1(nu + 3, 8), scan([(perm[2], 0), (perm[2], 1)]))
    f["a record outside the index and a record"] = (rec1(nu, 8), rec1(perm[2], 4))
    f["two records, one unitig"] = (rec1(perm[6], 5), rec1(perm[6], 9))
    f["two records, two unitigs"] = (rec1(perm[6], 5), rec1(perm[8], 9))
    f["a record and nothing found"] = (rec1(perm[6], 5), ("none", 12))
    f["nothing found and a scanned mate"] = (("none", 3), scan(walk(rng, perm[20:25])))
    f["a scanned mate and a mate without k-mers"] = (scan(walk(rng, perm[30:33])), scan([]))
    f["a mate without k-mers and a record"] = (scan([]), rec1(perm[12], 3))
    f["absent slots only"] = (scan([A] * 5), scan([A] * 70))
    f["nothing at all"] = (scan([]), scan([]))
    return f


def build_batch(p, rng, frags, mode):
    """the fragments as a batch that has run in text mode 1 or 2, its records and pairs overwritten.  Returns (batch, pairs, nks)"""
    k = 31
    recs, pairs, nks = [], [], []
    for mates in frags:
        for m in mates:
            r = np.zeros(1, dtype=fa.RECORD_DTYPE)[0]
            if m[0] == "scan":
                slots = m[1]
                r["nk"] = len(slots)   # (as fin_batch_download_records delivers a searched read; inject zeroes it for the device)
            elif m[0] == "rec":
                slots = [(m[1], i) for i in range(m[2])]
                r["u"], r["nk"], r["meta"] = m[1], m[2], 1 << 16
            else:
                slots = [(-1, -1)] * m[1]
                r["nk"], r["meta"] = m[1], 2 << 16
            recs.append(r); pairs += slots; nks.append(len(slots))
    recs = np.array(recs, dtype=fa.RECORD_DTYPE)
    pairs = np.array(pairs, dtype=np.int32).reshape(-1, 2)
    nks = np.array(nks, dtype=np.int64)
    reads = [random_genome(rng, int(n) + k - 1) if n else "ACGT" for n in nks]
    b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(pairs) and b.n_reads == len(recs)
    if len(recs):
        inject(b, recs, pairs, mode)
    return b, pairs, nks


@pytest.mark.parametrize("n_colors", [40, 130])
@pytest.mark.parametrize("mode", [1, 2])
def test_hand_made_fragments(wide, mode, n_colors):
    """records and pairs made by hand (set_records): seeds, the table's limit on the FRAGMENT, rows of 64 slots, places outside the index -- and F = 1, 65 and 257,
    the wave's and the block's edge, with every case somewhere in every wave"""
    p, rng = wide
    nu = p.n_unitigs
    cases = hand_made_fragments(rng, nu)
    names = list(cases)
    bits = random_matrix(rng, nu, n_colors, empty_share=0.15)
    col = p.colors(n_colors, bits)
    for F in (len(names), 1, 65, 257):
        order = names if F == len(names) else [names[int(i)] for i in rng.integers(0, len(names), F)]
        b, pairs, nks = build_batch(p, rng, [cases[n] for n in order], mode)
        for pm in (0, 300, 500, 1000):
            want = frags_of(pairs, nks, bits, n_colors, pm)
            for both in (False, True):
                rows, heads = b.pseudoalign_pairs(col, pm, both)
                wr, wh = only_both(want) if both else want
                for i, n in enumerate(order):
                    assert tuple(heads[i].tolist()) == tuple(wh[i].tolist()) and np.array_equal(rows[i], wr[i]), \
                        "F=%d, fragment %d (%s), %d colours, permille %d, both %s: got %s %s, want %s %s" % (F, i, n, n_colors, pm, both, heads[i], rows[i], wh[i], wr[i])
        b.close()
    col.close()


def test_two_records_at_the_thresholds(wide):
    """the closed form as the DEVICE computes it: two kind-1 mates of na and nb slots in unitigs with different non-empty rows (and one with an empty row), at
    the thresholds on both sides of 1000 na / (na + nb) and 1000 nb / (na + nb), where the 64-bit comparison decides; W = 1 (a lane by itself) and W = 3 (the
    wave-cooperative form)"""
    p, rng = wide
    nu = p.n_unitigs
    counts = [(1, 2), (2, 1), (3, 7), (7, 3), (1, 6), (6, 1), (5, 5), (4, 6), (1, 1), (9, 11)]
    pms = sorted({0, 1000} | {int(x) for na, nb in counts for c in (na, nb) for x in (1000 * c // (na + nb), 1000 * c // (na + nb) + 1) if x <= 1000})
    assert {333, 334, 666, 667, 300, 301, 700, 701, 142, 143, 857, 858, 450, 451} <= set(pms)
    for mode, n_colors in ((1, 40), (2, 130)):
        bits = random_matrix(rng, nu, n_colors, empty_share=0.15)
        x, y, z, e = (int(u) for u in rng.permutation(nu)[:4])
        top = n_colors - 1   # x and y: neither row inside the other, so all three terms of the form are met; z inside x; e empty
        for u, cs in ((x, [0, 1, top]), (y, [1, 2, top - 1]), (z, [0, 1]), (e, [])):
            bits[u] = pack([cs], n_colors)[0]
        frags = [(rec1(ua, na), rec1(ub, nb)) for na, nb in counts for ua, ub in ((x, y), (x, z), (x, x), (x, e), (e, y))]
        b, pairs, nks = build_batch(p, rng, frags, mode)
        col = p.colors(n_colors, bits)
        changes = 0
        last = None
        for pm in pms:
            want = frags_of(pairs, nks, bits, n_colors, pm)
            assert_frags(b.pseudoalign_pairs(col, pm), want, "two records, %d colours, permille %d" % (n_colors, pm))
            assert_frags(b.pseudoalign_pairs(col, pm, both=True), only_both(want), "two records, %d colours, permille %d, both" % (n_colors, pm))
            changes += last is not None and not np.array_equal(last, want[0])
            last = want[0]
        assert changes >= 10, "the thresholds do not decide anything"
        b.close(); col.close()


def test_no_fragments(wide):
    p, rng = wide
    col = p.colors(70)
    b = p.batch([]); b.text_mode(2); b.run(fa.FIN_MERGED)
    rows, heads = b.pseudoalign_pairs(col)
    assert rows.shape == (0, 2) and len(heads) == 0
    eq = col.eqclasses(16)
    assert eq.add_pairs(b).stats()[:3] == [0, 0, 0]
    rows, heads, npos = p.pseudoalign_pairs([], col)
    assert rows.shape == (0, 2) and len(heads) == 0 and npos == 0
    assert eq.add_read_pairs([]).stats()[:3] == [0, 0, 0]
    b.close(); eq.close(); col.close()


# ---- classes, abundances, host buffers, streams --------------------------------------------------------------------------------------------
def test_classes_and_abundances_of_fragments(w):
    """a fragment is one row and one "read" of its class: EqClasses.add_pairs against np.unique over the expected rows; the estimate over that accumulator against
    the model and against classes_abundance over its own download, one iteration under RTOL1"""
    n = 65
    for mode, pm, both in ((2, 1000, False), (0, 300, True)):
        want_rows = (only_both(w.want[n][pm]) if both else w.want[n][pm])[0]
        want = classes_of_rows(want_rows, n)
        assert len(want[0]) >= 4 and want[2] > 0
        eq = w.cols[n].eqclasses(4096)
        b = w.p.batch(w.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        eq.add_pairs(b, pm, both)
        what = "k=%d text mode %d, permille %d, both %s" % (w.k, mode, pm, both)
        assert_classes(eq.download(), want, what)
        assert eq.stats()[:3] == [len(w.reads) // 2, want[2], len(want[0])], what
        crows, creads, _ = eq.download()
        got = eq.abundance(max_iters=1, tol=0.0, trace=True)
        assert got.n_reads == int(want[1].sum()) and got.n_unaligned == want[2]
        assert_one_iteration(got, Model(crows, creads, n).run(1, 0.0), len(crows), n, what)
        host = fa.classes_abundance(crows, creads, n, max_iters=1, tol=0.0)
        assert (np.abs(got.alpha - host.alpha) <= rtol1(len(crows), n) * np.abs(host.alpha)).all(), what + ": against classes_abundance"
        eq.add_pairs(b, pm, both)   # adding twice counts twice
        assert_classes(eq.download(), (want[0], want[1] * np.uint64(2), 2 * want[2]), what + ", twice")
        b.close(); eq.close()


def test_host_buffers_cut_between_pairs_only(w):
    """801 fragments whose k-mers are cut into at least 5 sub-batches: rows, heads and classes equal the one-batch expectation, so no pair was split"""
    n, p = 130, w.p
    rd = (w.reads + w.reads)[:1602]
    assert len(rd) == 1602
    nk = nks_of(rd, w.k)
    e1 = oracle_pairs(w.o, rd)
    want = {pm: frags_of(e1, nk, w.mats[n], n, pm) for pm in (1000, 300)}
    rows, heads, npos = p.pseudoalign_pairs(rd, w.cols[n])
    assert_frags((rows, heads), want[1000], "host buffers, one sub-batch")
    assert npos == int(want[1000][1]["n_colored"].sum()) > 0
    limit = int(nk.sum()) // 7
    at = np.concatenate([[0], np.cumsum(nk)])
    cuts = np.searchsorted(at, np.arange(1, 7) * limit)   # where cuts by single reads would fall: some of them inside a pair
    assert int(nk.sum()) // limit >= 5 and (cuts % 2 == 1).any()
    eq = w.cols[n].eqclasses(4096)
    p.set_option("pipeline_kmers", limit); p.set_option("pipeline_depth", 3)
    try:
        for pm, both in ((1000, False), (300, True)):
            wt = only_both(want[pm]) if both else want[pm]
            rows, heads, npos = p.pseudoalign_pairs(rd, w.cols[n], pm, both)
            assert_frags((rows, heads), wt, "host buffers, sub-batches, permille %d" % pm)
            assert npos == int(wt[1]["n_colored"].sum())
            none, heads2, npos2 = p.pseudoalign_pairs(rd, w.cols[n], pm, both, want_rows=False)
            assert none is None and heads2.tobytes() == wt[1].tobytes() and npos2 == npos
            assert_classes(eq.reset().add_read_pairs(rd, pm, both).download(), classes_of_rows(wt[0], n), "classes from host buffers, permille %d" % pm)
    finally:
        p.set_option("pipeline_kmers", None); p.set_option("pipeline_depth", None)
    for call in (lambda: p.pseudoalign_pairs(rd[:11], w.cols[n]), lambda: eq.add_read_pairs(rd[:11])):   # an odd number of reads, before anything runs
        with pytest.raises(fa.FinitoError) as e:
            call()
        assert e.value.code == fa.FIN_EINVAL and "odd" in str(e.value)
    eq.close()


def test_refusals_on_the_device(w):
    p, col = w.p, w.cols[5]
    b = p.batch(w.reads[:50])
    eq = col.eqclasses(64)
    for call in (lambda: b.pseudoalign_pairs(col), lambda: eq.add_pairs(b)):   # a batch that has not run
        with pytest.raises(fa.FinitoError) as e:
            call()
        assert e.value.code == fa.FIN_EINVAL
    b.run(fa.FIN_MERGED)
    L, err = fa.lib(), fa.C.create_string_buffer(512)
    for mode in (2, 0xFFFFFFFF):
        assert L.fin_batch_pseudoalign_paired(b.h, col.h, 1000, mode, err, 512) == fa.FIN_EINVAL and b"FIN_PAIR" in err.value
        assert L.fin_batch_add_eqclasses_paired(b.h, eq.h, 1000, mode, None, err, 512) == fa.FIN_EINVAL
    with pytest.raises(fa.FinitoError) as e:
        b.pseudoalign_pairs(col, 1001)
    assert e.value.code == fa.FIN_EINVAL and b.device_pair_ptrs() == (0, 0) and eq.stats()[0] == 0
    p2 = fa.FinimizerIndex.build(w.unitigs, w.k).to_device(0)
    foreign = p2.colors(5)
    for call in (lambda: b.pseudoalign_pairs(foreign), lambda: p.pseudoalign_pairs(w.reads[:10], foreign)):   # colours of another index
        with pytest.raises(fa.FinitoError) as e:
            call()
        assert e.value.code == fa.FIN_EINVAL
    foreign.close(); p2.close(); eq.close(); b.close()


def test_the_download_waits_for_an_add_of_fragments_behind_a_delay(w):
    """tests/test_streams.py's download case: the add of the fragments' rows sits behind a delay on a non-blocking stream when the download is issued"""
    n, pm = 64, 1000
    want = classes_of_rows(w.want[n][pm][0], n)
    b = w.p.batch(w.reads); b.text_mode(2); b.run(fa.FIN_MERGED)
    b.pseudoalign_pairs(w.cols[n], pm)   # (the run's overflow verdict is known: the add below has nothing to wait for)
    eq = w.cols[n].eqclasses(4096)
    eq.stats()
    delay, S = Delay(), torch.cuda.Stream()
    delay(S, 60.0)
    eq.add_pairs(b, pm, stream=S.cuda_stream)
    assert S.query() is False, "the stream is idle where its delay should still run"
    assert_classes(eq.download(), want, "behind a delay")
    b.close(); eq.close()
