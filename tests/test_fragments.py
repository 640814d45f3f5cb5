"""Fragment geometry on the device (include/finito_amd.h: FRAGMENT GEOMETRY, fin_batch_add_fragments, fin_batch_fragments, fin_search_batch_*fragments;
fin_fragments.hip).  The expectation is always tests/test_fragments_host.py's model -- plain Python from the header's definition -- over the
ORACLE's pairs or over hand-made pairs (a record's slots by tests/test_records.py::brute_expand), never a device output or a fin_records_* result; every
comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import finito_amd as fa
from oracle.oracle import OracleIndex
from tests.test_fragments_host import INWARD, ONE, assert_frags, assert_stats, build, fragments_model, mate, stats_of
from tests.test_records import brute_expand
from tests.test_records_device import inject
from tests.test_segments import nks_of, oracle_pairs
from tests.test_streams import Delay
from tests.test_unitig_counts import read_families
from tests.test_unitig_depth import device_int32
from tests.util import cut_unitigs, random_genome, rc, sample_reads

pytestmark = pytest.mark.gpu

CONFIGS = ((1, 1), (64, 7), (1024, 1), (4096, 1))


def nine_substitutions(read, k):
    """a read of k + 59 bases with nine substitutions less than k apart that leave its first two k-mers alone and no other: more than the fast path settles, so the
    pipeline searches the read, and still straight"""
    assert len(read) == k + 59
    r = list(read)
    for j in range(9):
        p = k + 1 + 7 * j
        r[p] = "ACGT"[("ACGT".index(r[p]) + 1 + j % 3) % 4]
    return "".join(r)


def chosen_fragments(unitigs, k, rng):
    """fragments cut from ONE unitig at chosen geometry, every one as (exact, exact), (exact, nine substitutions), (nine, exact), (nine, nine); fragments over two
    unitigs; a placed mate beside a read from nowhere"""
    Lr = k + 59
    long = [u for u in unitigs if len(u) >= 2 * Lr + 30][:40]
    assert len(long) >= 24
    out = []
    for i, u in enumerate(long):
        a, b = 3, len(u) - Lr - 2
        A, B, A7 = u[a:a + Lr], u[b:b + Lr], u[a:a + Lr + 7]
        fwd = lambda s, sub: nine_substitutions(s, k) if sub else s
        # a reverse mate with substitutions: they go into the read as it is sequenced, so strand A has them mirrored
        rev = lambda s, sub: nine_substitutions(rc(s), k) if sub else rc(s)
        for sa in (0, 1):
            for sb in (0, 1):
                out += [fwd(A, sa), rev(B, sb)]                     # inward
                out += [rev(B, sa), fwd(A, sb)]                     # inward, the reverse mate first
                out += [fwd(B, sa), rev(A, sb)]                     # outward
                out += [fwd(A, sa), fwd(B, sb)]                     # tandem, forward
                out += [rev(A, sa), rev(B, sb)]                     # tandem, reverse
                out += [fwd(A, sa), rc(A7) if not sb else rev(A, 1)]   # equal starts: inward by the first condition's equality
        v = long[(i + 1) % len(long)]
        out += [A7, rc(A), rc(A), A7]                                # the reverse mate inside the forward one, equal starts: outward by the second condition alone
        out += [A, rc(v[5:5 + Lr]), nine_substitutions(A, k), v[5:5 + Lr]]   # two unitigs
        out += [A, random_genome(rng, Lr), random_genome(rng, 40), rev(B, 1)]   # one mate from nowhere
    return out


class World:
    def __init__(self, k):
        self.k = k
        rng = self.rng = np.random.default_rng(4000 + k)
        g = self.g = random_genome(rng, 40000)
        self.unitigs = cut_unitigs(rng, g, k, max_len=max(700, 4 * k))
        self.p = fa.FinimizerIndex.build(self.unitigs, k).to_device(0)
        self.o = OracleIndex.build(self.unitigs, k)
        self.ends = self.o.ends()
        assert np.array_equal(self.p.export(fa.X_ENDS), self.ends)
        fam = read_families(rng, g, k, self.unitigs, n=400)
        self.reads = chosen_fragments(self.unitigs, k, rng) + fam[: len(fam) & ~1]
        assert len(self.reads) % 2 == 0 and len(self.reads) >= 1200
        self.nks = nks_of(self.reads, k)
        self.pairs = oracle_pairs(self.o, self.reads)
        self.want = fragments_model(self.pairs, self.nks, k, self.ends)
        self.stats = {c: stats_of(self.want, *c) for c in CONFIGS}
        for a in (self.nks, self.pairs, self.want):
            a.setflags(write=False)

    def close(self):
        self.p.close()


@pytest.fixture(scope="module", params=[31, 127], ids=lambda k: "k%d" % k)
def w(request):
    world = World(request.param)
    yield world
    world.close()


def assert_expectation_shows_everything(w, recs=None):
    """the guards, asserted on the expectation (and, for the routes, on the records the step left: the input, not a result)"""
    cls = w.want["cls"] & 0xFF
    counts = np.bincount(cls, minlength=6)
    assert (counts >= 8).all(), "a class with fewer than 8 members: %s" % counts
    assert len(w.want) >= 600
    lens = w.want["length"][cls == INWARD]
    assert (lens // 7 > 63).any() and (lens // 7 < 63).any(), "no inward length saturates 64 bins of 7, or all do"
    assert w.stats[(1024, 1)][0][-1] == 0 and w.stats[(64, 7)][0][-1] > 0 and w.stats[(1, 1)][0][0] == counts[INWARD]
    if recs is not None:
        ka, kb = (recs["meta"][0::2] >> 16), (recs["meta"][1::2] >> 16)
        inward = cls == INWARD
        routes = {"record + record": (inward & (ka == 1) & (kb == 1)).sum(), "record + scan": (inward & (ka == 1) & (kb == 0)).sum(),
                  "scan + record": (inward & (ka == 0) & (kb == 1)).sum(), "scan + scan": (inward & (ka == 0) & (kb == 0)).sum()}
        assert all(v >= 8 for v in routes.values()), "inward fragments by route: %s" % routes
        scanned = np.nonzero((ka == 0) | (kb == 0))[0]
        assert (np.bincount(scanned // 64) >= 2).any(), "no wave holds several scanned mates"


def flagged_state(a):
    """(hist, counters) of an accumulator whose download refuses, read where they lie: uint64 hist[n_bins], then the seven counters (fin_fragments_device_hist)"""
    words = device_int32(a.device_ptr(), 2 * (a.n_bins + 7)).view(np.uint64)
    return words[: a.n_bins].copy(), words[a.n_bins:].copy()


def accumulators(p):
    return {c: p.fragments(*c) for c in CONFIGS}


def test_fragments_and_accumulators_in_every_text_mode(w):
    """text modes 0 (no records), 1 and 2 (records where k <= 63; k = 127 leaves none: every mate is scanned): the per-fragment output and the accumulator under
    four (n_bins, bin_width) against the model; adding twice doubles; reset zeroes; what forgets the read summaries forgets the fragments; an odd batch"""
    k, p = w.k, w.p
    assert_expectation_shows_everything(w)
    accs = accumulators(p)
    for mode in (0, 1, 2):
        what = "k=%d text mode %d" % (k, mode)
        b = p.batch(w.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        assert b.device_fragments_ptr() == 0
        info = b.run_info()
        if k <= 63 and mode:
            assert info["fast_path"] and b.pipeline_counts()[41] > 0
            assert_expectation_shows_everything(w, b.records()[0])
        elif k > 63:
            assert not info["fast_path"]
        assert_frags(b.fragments(), w.want, what)
        assert b.device_fragments_ptr() != 0
        for c, a in accs.items():
            a.reset().add(b)
            assert_stats((a.download().hist, a.download().counters), w.stats[c], "%s, %d bins of %d" % (what, *c))
            a.add(b)
            st = a.download()
            assert_stats((st.hist, st.counters), (w.stats[c][0] * np.uint64(2), w.stats[c][1] * np.uint64(2)), "%s, %d bins of %d, twice" % (what, *c))
            st = a.reset().download()
            assert not st.hist.any() and not st.counters.any() and st.n_fragments == 0 and st.mean is None and st.quantile(500) is None
        b.read_summaries()
        assert_frags(b.fragments(), w.want, what + ", again")
        b.reload(w.reads[:51])
        assert b.device_fragments_ptr() == 0
        b.run(fa.FIN_MERGED)
        for call in (b.fragments, lambda: accs[(64, 7)].add(b)):
            with pytest.raises(fa.FinitoError) as e:
                call()
            assert e.value.code == fa.FIN_EINVAL and "odd" in str(e.value)
        assert b.device_fragments_ptr() == 0 and not accs[(64, 7)].download().counters.any()
        b.close()
    for a in accs.values():
        a.close()


def test_the_statistics_of_a_download(w):
    a = w.p.fragments(1024, 1)
    b = w.p.batch(w.reads); b.text_mode(2); b.run(fa.FIN_MERGED)
    st = a.add(b).download()
    hist, counters = w.stats[(1024, 1)]
    lens = np.sort(w.want["length"][(w.want["cls"] & 0xFF) == INWARD].astype(np.int64))
    assert [st.none, st.one, st.split, st.tandem, st.outward, st.inward] == counters[:6].tolist() and st.n_fragments == len(w.want) and st.len_sum == int(lens.sum())
    assert st.mean == int(lens.sum()) / len(lens)
    for pm in (0, 1, 500, 999, 1000):
        t = max(1, -(-pm * len(lens) // 1000))
        assert st.quantile(pm) == (int(lens[t - 1]), False)
    ref = [10, 100, 150, 400, 1000, 10**6]
    got = st.effective_lengths(ref)
    for r, g in zip(ref, got):
        fit = lens[lens <= r]
        assert g == (float(r) + 1.0 - float(fit.sum()) / float(len(fit)) if len(fit) else float(r))
    assert got[0] == 10.0 and got[-1] == 10**6 + 1.0 - st.mean
    a.close(); b.close()


# ---- hand-made records and pairs ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    k = 31
    rng = np.random.default_rng(4064)
    g = random_genome(rng, 12000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, k, max_len=80), k).to_device(0)
    assert p.n_unitigs >= 200
    yield p, rng, p.export(fa.X_ENDS)
    p.close()


def hand_made_mates(rng, ends, k, n, as_records):
    """2n mates over the unitigs with at least 30 k-mers: straight ones on either strand, as kind-1 records (with up to eight positions) or as scanned reads (with
    absent slots); a few unitigs only, so that two mates often share one.  as_records False: every mate is a scanned read holding the SAME slots"""
    lens = np.diff(np.concatenate([[0], ends]))
    us = [int(u) for u in np.nonzero(lens - k + 1 >= 30)[0][:2]]
    out = []
    for _ in range(2 * n):
        t = rng.random()
        u = us[int(rng.integers(0, 2))]; nk = int(rng.integers(1, 14)); rev = bool(rng.integers(0, 2))
        s0 = int(rng.integers(0, lens[u] - k + 1 - nk + 1))
        if t < 0.05:
            out.append(("none", nk))
        elif t < 0.1:
            out.append(("scan", []))
        elif t < 0.15:
            out.append(("scan", mate(u, s0, nk, rev)[1] + [(us[0], 0)]))   # a mosaic, or an indel
        else:
            Es = sorted(int(x) for x in rng.integers(0, nk + k - 1, int(rng.integers(0, 9)))) if rng.random() < 0.3 else []
            out.append(mate(u, s0, nk, rev, "rec", Es))
    if not as_records:
        recs, stream = build(out)
        pairs = brute_expand(recs, stream, k).tolist()
        at = np.concatenate([[0], np.cumsum(recs["nk"].astype(np.int64))])
        out = [("scan", [tuple(x) for x in pairs[at[r]:at[r + 1]]]) for r in range(len(recs))]
    return out


def batch_of(p, rng, mates, k, mode):
    """the mates as a batch that has run in text mode 1 or 2, its records and pairs overwritten.  Returns (batch, the model's fragments)"""
    recs, stream = build(mates)
    pairs = brute_expand(recs, stream, k)
    nks = recs["nk"].astype(np.int64)
    reads = [random_genome(rng, int(n) + k - 1) if n else "ACGT" for n in nks]
    b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(pairs) and b.n_reads == len(recs)
    inject(b, recs, pairs, mode)
    return b, pairs, nks


@pytest.mark.parametrize("mode", [1, 2])
def test_hand_made_records_and_the_same_slots_scanned(wide, mode):
    """records made by hand (set_records) -- positions that leave two, one or no found slot, either strand, mates that share a unitig -- and the SAME slots as
    scanned reads: the record route and the scan route both equal the model, at F = 1, 65 and 257 and 600: the wave's and the block's edges"""
    p, rng, ends = wide
    k = 31
    a = p.fragments(64, 1)
    for F in (1, 65, 257, 600):
        seed = 4100 + 10 * F + mode   # (fixed: the guard below is checked on the model alone)
        want = None
        for as_records in (True, False):
            mates = hand_made_mates(np.random.default_rng(seed), ends, k, F, as_records)
            b, pairs, nks = batch_of(p, rng, mates, k, mode)
            model = fragments_model(pairs, nks, k, ends)
            if want is None:
                want = model
                if F == 600:
                    assert (np.bincount(want["cls"] & 0xFF, minlength=6) >= 8).all()
            assert model.tobytes() == want.tobytes(), "the two forms of the input differ"
            what = "F=%d, mode %d, %s" % (F, mode, "records" if as_records else "scanned")
            assert_frags(b.fragments(), want, what)
            st = a.reset().add(b).download()
            assert_stats((st.hist, st.counters), stats_of(want, 64, 1), what)
            b.close()
    a.close()


def test_a_place_outside_the_index_is_flagged_and_not_placed(wide):
    p, rng, ends = wide
    k, nu = 31, p.n_unitigs
    lens = np.diff(np.concatenate([[0], ends]))
    u = int(np.nonzero(lens - k + 1 >= 30)[0][0])
    good = mate(u, 2, 9, True, "rec")
    cases = {"a record outside the index": mate(nu + 3, 0, 6, False, "rec"), "a record that hangs over its unitig's end": mate(u, int(lens[u]) - k - 2, 9, False, "rec"),
             "a scanned slot outside the index": ("scan", [(nu, 0), (nu, 1), (nu, 2)]), "a scanned slot at 0x7FFFFFFF": ("scan", [(u, 0), (u, 1), (0x7FFFFFFF, 2)])}
    a = p.fragments(64, 1)
    for name, bad in cases.items():
        for first in (True, False):
            mates = [mate(u, 0, 5, False, "rec"), good] * 70 + ([bad, good] if first else [good, bad])
            b, pairs, nks = batch_of(p, rng, mates, k, 1)
            want = fragments_model(pairs, nks, k, ends)
            assert want["cls"][-1] == (ONE | (0xA00 if first else 0x500)) and (want["cls"][:-1] & 0xFF == INWARD).all()
            assert_frags(b.fragments(), want, name)
            a.add(b)
            for _ in range(2):
                with pytest.raises(fa.FinitoError) as e:
                    a.download()
                assert e.value.code == fa.FIN_EINVAL and "outside the index" in str(e.value), name
            assert_stats(flagged_state(a), stats_of(want, 64, 1), name + ": behind the refusing download, that mate counted as not placed")
            st = a.reset().download()
            assert not st.counters.any(), name
            b.close()
    a.close()


# ---- streams, refusals, host buffers ---------------------------------------------------------------------------------------------------------------
def test_the_download_waits_for_an_add_behind_a_delay(w):
    b = w.p.batch(w.reads); b.text_mode(2); b.run(fa.FIN_MERGED)
    b.fragments()   # (the run's overflow verdict is known: the add below has nothing to wait for)
    a = w.p.fragments(64, 7)
    a.download()
    delay, S = Delay(), torch.cuda.Stream()
    delay(S, 60.0)
    a.add(b, stream=S.cuda_stream)
    assert S.query() is False, "the stream is idle where its delay should still run"
    st = a.download()
    assert_stats((st.hist, st.counters), w.stats[(64, 7)], "behind a delay")
    a.close(); b.close()


def test_refusals_and_sentinels_through_the_c_abi(w):
    p = w.p
    L, err = fa.lib(), C.create_string_buffer(512)
    h = C.c_void_p()
    for nb, bw in ((0, 1), (4097, 1), (64, 0)):
        assert L.fin_fragments_create(p.h, 0, nb, bw, C.byref(h), err, 512) == fa.FIN_EINVAL and not h.value
        with pytest.raises(fa.FinitoError):
            p.fragments(nb, bw)
    assert L.fin_fragments_create(p.h, 1 << 20, 64, 1, C.byref(h), err, 512) == fa.FIN_ENODEV, "a device without a replica"
    b = p.batch(w.reads[:50])
    a = p.fragments(64, 7)
    for call in (b.fragments, lambda: a.add(b)):   # a batch that has not run
        with pytest.raises(fa.FinitoError) as e:
            call()
        assert e.value.code == fa.FIN_EINVAL
    b.run(fa.FIN_MERGED)
    assert L.fin_batch_download_fragments(b.h, None, err, 512) == fa.FIN_EINVAL and b"fin_batch_fragments first" in err.value
    p2 = fa.FinimizerIndex.build(w.unitigs, w.k).to_device(0)
    foreign = p2.fragments(64, 7)
    with pytest.raises(fa.FinitoError) as e:   # an accumulator of another index
        foreign.add(b)
    assert e.value.code == fa.FIN_EINVAL and "different indexes" in str(e.value)
    assert L.fin_search_batch_add_fragments(p.h, *fa._reads_args(w.reads[:10]), fa.FIN_MERGED, foreign.h, err, 512) == fa.FIN_EINVAL and b"another index" in err.value
    assert not foreign.download().counters.any()
    foreign.close(); p2.close()
    # a sentinel behind every output buffer
    SENT = 0xA5A5A5A5A5A5A5A5
    nf = 25
    out = np.full(nf * 2 + 2, SENT, dtype=np.uint64)
    n = C.c_uint64(0)
    fa._check(L.fin_batch_fragments(b.h, C.byref(n), err, 512), err)
    fa._check(L.fin_batch_download_fragments(b.h, out.ctypes.data_as(C.c_void_p), err, 512), err)
    want = fragments_model(w.pairs[: int(w.nks[:50].sum())], w.nks[:50], w.k, w.ends)
    assert n.value == nf and out[:-2].tobytes() == want.tobytes() and (out[-2:] == SENT).all()
    a.add(b)
    hist, counters = np.full(65, SENT, dtype=np.uint64), np.full(8, SENT, dtype=np.uint64)
    fa._check(L.fin_fragments_download(a.h, hist.ctypes.data_as(C.c_void_p), counters.ctypes.data_as(C.c_void_p), err, 512), err)
    assert_stats((hist[:64], counters[:7]), stats_of(want, 64, 7), "the first 25 fragments")
    assert hist[64] == SENT and counters[7] == SENT
    out = np.full(nf * 2 + 2, SENT, dtype=np.uint64)
    fa._check(L.fin_search_batch_fragments(p.h, *fa._reads_args(w.reads[:50]), fa.FIN_MERGED, out.ctypes.data_as(C.c_void_p), err, 512), err)
    assert out[:-2].tobytes() == want.tobytes() and (out[-2:] == SENT).all()
    a.close(); b.close()


def test_host_buffers_cut_between_pairs_only(w):
    """the reads cut into at least five sub-batches at a limit that would cut a pair if reads were taken one by one: fragments and accumulator equal the one-batch
    expectation"""
    p = w.p
    nk = w.nks
    assert_frags(p.fragments_reads(w.reads), w.want, "host buffers, one sub-batch")
    limit = int(nk.sum()) // 7
    at = np.concatenate([[0], np.cumsum(nk)])
    cuts = np.searchsorted(at, np.arange(1, 7) * limit)   # where cuts by single reads would fall: some of them inside a pair
    assert int(nk.sum()) // limit >= 5 and (cuts % 2 == 1).any()
    a = p.fragments(64, 7)
    p.set_option("pipeline_kmers", limit); p.set_option("pipeline_depth", 3)
    try:
        assert_frags(p.fragments_reads(w.reads), w.want, "host buffers, sub-batches")
        st = a.add_reads(w.reads).download()
        assert_stats((st.hist, st.counters), w.stats[(64, 7)], "add_reads, sub-batches")
    finally:
        p.set_option("pipeline_kmers", None); p.set_option("pipeline_depth", None)
    for call in (lambda: p.fragments_reads(w.reads[:11]), lambda: a.add_reads(w.reads[:11])):   # an odd number of reads, before anything runs
        with pytest.raises(fa.FinitoError) as e:
            call()
        assert e.value.code == fa.FIN_EINVAL and "odd" in str(e.value)
    assert len(p.fragments_reads([])) == 0 and a.reset().add_reads([]).download().n_fragments == 0
    a.close()


def test_a_withheld_step_adds_nothing_and_is_reported_until_the_reset():
    """tests/test_pileup_records.py's recipe: with the overflow list cut to three entries a step of genome reads overruns; nobody has looked at its counter when the
    add is issued, so the kernel does: it adds nothing and flags the accumulator, the download reports FIN_ELIMIT until the reset, a good step after it equals the
    model"""
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    reads = sample_reads(rng, g, 500, 150)
    ends = p.export(fa.X_ENDS)
    pairs = p.search_reads(reads, fa.FIN_MERGED)[0]   # (before the options change; the pairs are the same under every option.  The model reads them as slots)
    want = fragments_model(pairs, nks_of(reads, k), k, ends)
    L = fa.lib()
    a = p.fragments(64, 7)
    try:
        assert L.fin_set_option(b"lds_deque_limit", 1) == 0 and L.fin_set_option(b"seed_anchors", 0) == 0 and L.fin_set_option(b"debug_ovf_cap", 3) == 0
        for mode in (0, 2):
            b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
            a.add(b)
            for _ in range(2):
                with pytest.raises(fa.FinitoError) as e:
                    a.download()
                assert e.value.code == fa.FIN_ELIMIT and "overflow list" in str(e.value)
            # what the reset clears, looked at before it: nothing was added
            hist, counters = flagged_state(a)
            assert not hist.any() and not counters.any(), "a withheld step added something (mode %d)" % mode
            st = a.reset().download()
            assert not st.hist.any() and not st.counters.any()
            with pytest.raises(fa.FinitoError) as e:   # the host knows now: fin_batch_fragments refuses, and so does the add
                b.fragments()
            assert e.value.code == fa.FIN_ELIMIT and b.device_fragments_ptr() == 0
            with pytest.raises(fa.FinitoError) as e:
                a.add(b)
            assert e.value.code == fa.FIN_ELIMIT
            assert not a.download().counters.any()
            b.close()
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        st = a.add(b).download()
        assert_stats((st.hist, st.counters), stats_of(want, 64, 7), "a good step after the reset")
        assert st.n_fragments == 250
        b.close()
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)
        a.close(); p.close()
