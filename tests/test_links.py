"""Links on the device (include/finito_amd.h: LINKS, fin_links_*, fin_batch_add_links, fin_search_batch_add_links; fin_links.hip).  The expectation is
always tests/test_links_host.py's Model -- plain Python from the header's definition -- over the ORACLE's pairs or over hand-made pairs (a record's slots by
tests/test_records.py::brute_expand), never a device output or a fin_records_* result; every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.test_fragments_host import build, mate
from tests.test_links_host import Model, assert_table
from tests.test_records import brute_expand
from tests.test_records_device import inject
from tests.test_segments import nks_of, oracle_pairs
from tests.test_streams import Delay
from tests.test_unitig_depth import device_int32
from tests.util import cut_unitigs, random_genome, rc, sample_reads

pytestmark = pytest.mark.gpu


def table_in_hbm(a):
    """{(g_a, g_b): count} read where it lies (fin_links_device_table), for an accumulator whose download refuses, and n_distinct"""
    words = device_int32(a.device_ptr(), 4 * a.capacity + 2).view(np.uint64)
    slots = words[: 2 * a.capacity].reshape(-1, 2)
    occ = slots[slots[:, 0] != np.uint64(0xFFFFFFFFFFFFFFFF)]
    return {(int(key) >> 32, int(key) & 0xFFFFFFFF): int(c) for key, c in occ}, int(words[2 * a.capacity])


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------------------------------
class World:
    def __init__(self, k):
        self.k = k
        rng = self.rng = np.random.default_rng(4290 + k)
        g = self.g = random_genome(rng, 40000)
        L = self.L = k + 60
        # a sequence that holds one (k-1)-mer twice: the read A + S + C has every k-mer in it, and steps from the first copy to the second
        A, S, B, Cc = (random_genome(rng, n) for n in (40, k - 1, 40, 40))
        self.unitigs = cut_unitigs(rng, g, k, max_len=max(150, 2 * k)) + [A + S + B + S + Cc]
        self.p = fa.FinimizerIndex.build(self.unitigs, k).to_device(0)
        self.o = OracleIndex.build(self.unitigs, k)
        self.ends = self.o.ends()
        assert np.array_equal(self.p.export(fa.X_ENDS), self.ends)
        tiled = [g[a:a + L] for a in range(0, 20000, 55)]                               # reads that cross the cuts: every k-mer of the first half
        inside = [u[:k + 19] for u in self.unitigs if len(u) >= k + 19][:30]            # exact reads inside one unitig: the fast path finishes them
        mosaics = [g[a:a + L // 2 + k] + g[b:b + L // 2 + k] for a, b in rng.integers(0, len(g) - L, (40, 2))]   # two places: k - 1 absent slots in between
        reads = tiled + [rc(r) for r in tiled[::3]] + inside + [rc(r) for r in inside[::2]] + mosaics + [random_genome(rng, L) for _ in range(20)]
        reads += [A + S + Cc, rc(A + S + Cc)] + sample_reads(rng, g, 60, L)
        self.reads = [reads[i] for i in rng.permutation(len(reads))]
        assert 300 <= len(self.reads) <= 900
        self.nks = nks_of(self.reads, k)
        self.pairs = oracle_pairs(self.o, self.reads)
        self.m = Model(self.pairs, self.nks, self.ends)
        for a in (self.nks, self.pairs):
            a.setflags(write=False)

    def close(self):
        self.p.close()


@pytest.fixture(scope="module", params=[31, 127], ids=lambda k: "k%d" % k)
def w(request):
    world = World(request.param)
    yield world
    world.close()


def assert_expectation_shows_everything(w):
    m = w.m
    assert m.n_distinct >= 200, "%d links" % m.n_distinct
    assert len(m.both_ways) >= 50, "%d links reached from both read orientations" % len(m.both_ways)
    assert m.same_unitig_jumps >= 1 and m.outside == 0
    assert max(m.counts.values()) >= 2


def test_links_of_a_run_with_records_and_without(w):
    """text mode 2 (records where k <= 63) and text mode 0 (no records; k = 127 never has any: every read is scanned): the same table, the model's; adding twice
    doubles every count; fin_search_batch_add_links over host buffers gives the same table, through several sub-batches too"""
    k, p = w.k, w.p
    assert_expectation_shows_everything(w)
    a = p.links(4096)
    assert a.capacity == 8192
    tables = {}
    for mode in (2, 0):
        what = "k=%d text mode %d" % (k, mode)
        b = p.batch(w.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        if k <= 63 and mode:
            assert b.run_info()["fast_path"]
            kinds = np.bincount(b.records()[0]["meta"] >> 16, minlength=3)
            assert (kinds >= 8).all(), "reads by record kind: %s" % kinds
        elif k > 63:
            assert not b.run_info()["fast_path"]
        tables[mode] = a.reset().add(b).download()
        assert_table(tables[mode], w.m, what)
        for mc in (2, 3, 10**6):
            assert_table(a.download(mc), w.m, what + ", min_count %d" % mc, mc)
        assert_table(a.add(b).download(), w.m, what + ", twice", times=2)
        assert_table(a.download(3), w.m, what + ", twice, min_count 3", 3, times=2)
        b.close()
    assert tables[0].links.tobytes() == tables[2].links.tobytes()
    e = tables[2].unitig_edges(w.ends, k)
    assert e.n_edge + e.n_jump == w.m.transitions and e.n_edge >= 200 and e.n_jump >= 1
    assert_table(a.reset().add_reads(w.reads).download(), w.m, "k=%d host buffers" % k)
    limit = int(w.nks.sum()) // 6
    p.set_option("pipeline_kmers", limit); p.set_option("pipeline_depth", 3)
    try:
        assert_table(a.reset().add_reads(w.reads).download(), w.m, "k=%d host buffers, sub-batches" % k)
    finally:
        p.set_option("pipeline_kmers", None); p.set_option("pipeline_depth", None)
    st = a.reset().add_reads([]).download()
    assert len(st.links) == 0 and (st.transitions, st.n_distinct, st.n_self) == (0, 0, 0)
    a.close()


# ---- 2. hand-made pairs, at the shapes where the scan can go wrong --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    k = 31
    rng = np.random.default_rng(4294)
    g = random_genome(rng, 12000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, k, max_len=80), k).to_device(0)
    assert p.n_unitigs >= 200
    yield p, rng, p.export(fa.X_ENDS)
    p.close()


def walk(ends, k, nk, jumps, u0):
    """nk slots that step by one inside a unitig -- the u0-th of those with at least four k-mers --, turning round at its ends (straight either way), except at the
    slots in `jumps`: there the read goes on at offset 1 of the next such unitig.  A jump at slot i is a transition between slots i - 1 and i"""
    kmers = np.diff(np.concatenate([[0], ends])) - k + 1
    roomy = np.nonzero(kmers >= 4)[0]
    assert len(roomy) >= 60
    at, off, d, out = u0 % len(roomy), 1, 1, []
    for i in range(nk):
        if i in jumps:
            at, off, d = (at + 1) % len(roomy), 1, 1
        elif i:
            if not 0 <= off + d < kmers[roomy[at]]:
                d = -d
            off += d
        out.append((int(roomy[at]), off))
    return ("scan", out)


def shape_cases(ends, k):
    """{name: [reads]} as build() takes them"""
    cases = {}
    for j, nk in enumerate((1, 2, 63, 64, 65, 128, 129)):
        u0 = 3 * j
        cases["nk %d, straight" % nk] = [walk(ends, k, nk, (), u0)]
        for name, at in (("slot 1", 1), ("63 -> 64", 64), ("127 -> 128", 128), ("the last slot", nk - 1)):
            if 1 <= at < nk:
                cases["nk %d, a transition at %s" % (nk, name)] = [walk(ends, k, nk, (at,), u0 + 1)]
        every = tuple(sorted({x for x in (1, 63, 64, 65, 127, 128, nk - 1) if 1 <= x < nk}))
        cases["nk %d, transitions at %s" % (nk, every)] = [walk(ends, k, nk, every, u0 + 2)]
    cases["read r ends and read r + 1 begins in found slots of different unitigs"] = [("scan", [(40, 1), (40, 2)]), ("scan", [(41, 3), (41, 4)]), ("scan", [(42, 0)]), ("scan", [(43, 0)])]
    cases["5, 6, 5, 6: straight both ways"] = [("scan", [(50, 5), (50, 6), (50, 5), (50, 6)])]
    cases["7, 7: a self link"] = [("scan", [(50, 7), (50, 7)])]
    cases["A -> B in one read, B -> A in another"] = [("scan", [(51, 2), (52, 3)]), ("scan", [(52, 3), (51, 2)])]
    cases["a kind-1 record whose expanded slots have gaps"] = [mate(53, 0, 20, False, "rec", (3, 40)), mate(54, 1, 18, True, "rec", (20,)), ("none", 7)]
    cases["an absent slot between two found ones"] = [("scan", [(55, 1), (-1, -1), (56, 1)]), ("scan", [(-1, -1), (55, 1), (56, 2), (-1, -1)])]
    return cases


def batch_of(p, rng, reads, k, mode):
    """the reads as a batch that has run in text mode 1 or 2, its records and pairs overwritten.  Returns (batch, pairs, nks)"""
    recs, stream = build(reads)
    pairs = brute_expand(recs, stream, k)
    nks = recs["nk"].astype(np.int64)
    b = p.batch([random_genome(rng, int(n) + k - 1) if n else "ACGT" for n in nks]); b.text_mode(mode); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(pairs) and b.n_reads == len(recs)
    inject(b, recs, pairs, mode)
    return b, pairs, nks


@pytest.mark.parametrize("mode", [1, 2])
def test_hand_made_pairs_each_case_alone_and_all_in_one_batch(wide, mode):
    p, rng, ends = wide
    k = 31
    cases = shape_cases(ends, k)
    a = p.links(1024)
    expect = {"5, 6, 5, 6: straight both ways": 0, "7, 7: a self link": 1, "A -> B in one read, B -> A in another": 2, "an absent slot between two found ones": 1,
              "a kind-1 record whose expanded slots have gaps": 0, "read r ends and read r + 1 begins in found slots of different unitigs": 0,
              "nk 129, a transition at 63 -> 64": 1, "nk 129, a transition at 127 -> 128": 1, "nk 65, a transition at the last slot": 1, "nk 1, straight": 0}
    for name, reads in cases.items():
        b, pairs, nks = batch_of(p, rng, reads, k, mode)
        m = Model(pairs, nks, ends)
        if name in expect:
            assert m.transitions == expect[name], name
        assert_table(a.reset().add(b).download(), m, "%s, mode %d" % (name, mode))
        b.close()
    assert Model(*batch_of_model(cases["A -> B in one read, B -> A in another"], k), ends).n_distinct == 1
    for order in (1, -1):
        reads = [r for name in list(cases)[::order] for r in cases[name]]
        b, pairs, nks = batch_of(p, rng, reads, k, mode)
        m = Model(pairs, nks, ends)
        assert m.transitions >= 30 and m.n_self == 1
        assert_table(a.reset().add(b).download(), m, "every case in one batch, order %d, mode %d" % (order, mode))
        b.close()
    a.close()


def batch_of_model(reads, k):
    recs, stream = build(reads)
    return brute_expand(recs, stream, k), recs["nk"].astype(np.int64)


# ---- 4. refusals and contracts ----------------------------------------------------------------------------------------------------------------------
def test_an_end_outside_the_index_is_flagged_and_not_counted(wide):
    p, rng, ends = wide
    k, nu = 31, p.n_unitigs
    last_len = int(ends[-1] - ends[-2])
    good = [walk(ends, k, 70, (1, 64, 69), 5), ("scan", [(7, 2), (9, 2)])]
    cases = {"a slot with u = n_unitigs": ("scan", [(3, 1), (nu, 0), (nu, 1), (4, 1)]), "a place at total_len": ("scan", [(3, 1), (nu - 1, last_len), (4, 1)])}
    a = p.links(64)
    for name, bad in cases.items():
        b, pairs, nks = batch_of(p, rng, good + [bad] + good, k, 1)
        m = Model(pairs, nks, ends)
        assert m.outside == 2 and m.transitions == 8, name
        a.reset().add(b)
        for _ in range(2):
            with pytest.raises(fa.FinitoError) as e:
                a.download()
            assert e.value.code == fa.FIN_EINVAL and "outside the index" in str(e.value), name
        assert table_in_hbm(a) == (m.counts, m.n_distinct), name + ": behind the refusing download, the other links are intact and nothing was counted for that slot"
        b.close()
        b, pairs, nks = batch_of(p, rng, good, k, 1)
        assert_table(a.reset().add(b).download(), Model(pairs, nks, ends), name + ": after the reset")
        b.close()
    a.close()


def test_a_withheld_step_adds_nothing_and_is_reported_until_the_reset():
    """tests/test_fragments.py's recipe: with the overflow list cut to three entries a step of genome reads overruns; nobody has looked at its counter when the add
    is issued, so the kernel does"""
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    reads = sample_reads(rng, g, 500, 150)
    ends = p.export(fa.X_ENDS)
    pairs = p.search_reads(reads, fa.FIN_MERGED)[0]   # (before the options change; the pairs are the same under every option.  The model reads them as slots)
    m = Model(pairs, nks_of(reads, k), ends)
    assert m.n_distinct >= 50
    L = fa.lib()
    a = p.links(4096)
    try:
        assert L.fin_set_option(b"lds_deque_limit", 1) == 0 and L.fin_set_option(b"seed_anchors", 0) == 0 and L.fin_set_option(b"debug_ovf_cap", 3) == 0
        for mode in (0, 2):
            b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
            a.add(b)
            for _ in range(2):
                with pytest.raises(fa.FinitoError) as e:
                    a.download()
                assert e.value.code == fa.FIN_ELIMIT and "overflow list" in str(e.value)
            assert table_in_hbm(a) == ({}, 0), "a withheld step added something (mode %d)" % mode
            assert len(a.reset().download().links) == 0
            b.close()
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        assert_table(a.add(b).download(), m, "a good step after the reset")
        b.close()
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)
        a.close(); p.close()


def test_refusals_through_the_c_abi(w):
    p = w.p
    L, err = fa.lib(), C.create_string_buffer(512)
    h = C.c_void_p()
    for bad in (0, (1 << 28) + 1, 1 << 40):
        assert L.fin_links_create(p.h, 0, bad, C.byref(h), err, 512) == fa.FIN_ELIMIT and not h.value and b"max_links" in err.value
        with pytest.raises(fa.FinitoError):
            p.links(bad)
    assert L.fin_links_create(p.h, 1 << 20, 64, C.byref(h), err, 512) == fa.FIN_ENODEV, "a device without a replica"
    assert L.fin_links_capacity(None) == 0 and not L.fin_links_device_table(None)
    L.fin_links_free(None)
    b = p.batch(w.reads[:50])
    a = p.links(4096)
    with pytest.raises(fa.FinitoError) as e:   # a batch that has not run
        a.add(b)
    assert e.value.code == fa.FIN_EINVAL and "has not run" in str(e.value)
    b.run(fa.FIN_MERGED)
    p2 = fa.FinimizerIndex.build(w.unitigs, w.k).to_device(0)
    foreign = p2.links(4096)
    with pytest.raises(fa.FinitoError) as e:   # an accumulator of another index
        foreign.add(b)
    assert e.value.code == fa.FIN_EINVAL and "different indexes" in str(e.value)
    assert L.fin_search_batch_add_links(p.h, *fa._reads_args(w.reads[:10]), fa.FIN_MERGED, foreign.h, err, 512) == fa.FIN_EINVAL and b"another index" in err.value
    assert len(foreign.download().links) == 0
    foreign.close(); p2.close()
    # n_links is wanted; a buffer one entry too small: FIN_ELIMIT, the true number, a sentinel behind the buffer untouched
    m = Model(w.pairs[: int(w.nks[:50].sum())], w.nks[:50], w.ends)
    assert m.n_distinct >= 5
    a.add(b)
    assert L.fin_links_download(a.h, 1, None, 0, None, None, err, 512) == fa.FIN_EINVAL
    n = C.c_uint64(0)
    out = np.full(3 * m.n_distinct, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    assert L.fin_links_download(a.h, 1, out.ctypes.data_as(C.c_void_p), m.n_distinct - 1, C.byref(n), None, err, 512) == fa.FIN_ELIMIT and n.value == m.n_distinct
    assert (out == 0xA5A5A5A5A5A5A5A5).all()
    cnt = np.zeros(5, dtype=np.uint64); cnt[4] = 0xA5
    fa._check(L.fin_links_download(a.h, 1, out.ctypes.data_as(C.c_void_p), m.n_distinct, C.byref(n), cnt.ctypes.data_as(C.c_void_p), err, 512), err)
    assert out.view(fa.LINK_DTYPE).tobytes() == m.table().tobytes() and cnt.tolist() == [m.transitions, m.n_distinct, m.n_distinct, m.n_self, 0xA5]
    a.close(); b.close()


def test_an_add_on_another_stream_is_ordered_behind_the_run_and_the_download_behind_the_add(w):
    a = w.p.links(4096)
    delay, S, T = Delay(), torch.cuda.Stream(), torch.cuda.Stream()
    b = w.p.batch(w.reads); b.text_mode(2)
    delay(S, 60.0)
    b.run(fa.FIN_MERGED, stream=S.cuda_stream)       # the run behind a delay on S, the add on T: ordered behind the run
    a.add(b, stream=T.cuda_stream)
    assert S.query() is False, "the stream is idle where its delay should still run"
    assert_table(a.download(), w.m, "the add on another stream than the run")
    delay(T, 60.0)
    a.add(b, stream=T.cuda_stream)                   # the add behind a delay: the download waits for it
    assert T.query() is False, "the stream is idle where its delay should still run"
    assert_table(a.download(), w.m, "the download behind a delayed add", times=2)
    a.close(); b.close()
