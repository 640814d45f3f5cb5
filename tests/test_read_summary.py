"""Per-read summaries and the screen, on the device (include/finito_amd.h: fin_batch_read_summaries, fin_batch_screen, fin_search_batch_read_summaries,
fin_search_batch_screen; fin_readsum.hip).  The expectation is always the definition written in numpy (tests/test_read_summary_host.py::summaries_of) over the
ORACLE's pairs -- or, for hand-made records and hand-made pairs, over those pairs -- never a device output or a fin_records_* result; every comparison is exact."""
import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import OracleIndex, format_pairs
from tests.test_read_summary_host import assert_summaries, rule, summaries_of
from tests.test_records import brute_expand
from tests.test_records_device import inject
from tests.test_segments import nks_of, oracle_pairs
from tests.test_segments_host import assert_segments, segments_of
from tests.test_unitig_counts import read_families
from tests.util import cut_unitigs, hand_made_case, random_genome, sample_reads, unpack_bits

pytestmark = pytest.mark.gpu

SCREENS = [(1, 0, 0), (0, 0, 0), (1, 0, 1), (10, 500, 0), (0, 1000, 0), (0, 1000, 1)]   # (min_found, min_permille, invert)


def expected(o, reads, k, strands=fa.FIN_MERGED):
    return summaries_of(oracle_pairs(o, reads, strands), nks_of(reads, k))


def run_summaries(p, reads, mode=0, strands=fa.FIN_MERGED):
    b = p.batch(reads); b.text_mode(mode); b.run(strands)
    got = b.read_summaries()
    b.close()
    return got


def assert_screen(got, want_rule, what=""):
    """got = (ids, bits) of a screen over len(want_rule) reads"""
    ids, bits = got
    n = len(want_rule)
    assert ids.dtype == np.uint32 and bits.dtype == np.uint64 and len(bits) == (n + 63) // 64, what
    assert np.array_equal(ids, np.nonzero(want_rule)[0]), "%s: ids" % what
    every = unpack_bits(bits, 64 * len(bits))
    assert np.array_equal(every[:n].astype(bool), want_rule), "%s: bits" % what
    assert not every[n:].any(), "%s: a bit at or beyond n_reads is set" % what


@pytest.fixture(scope="module")
def set31():
    rng = np.random.default_rng(20414)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, 31, max_len=700)
    p = fa.FinimizerIndex.build(unitigs, 31).to_device(0)
    o = OracleIndex.build(unitigs, 31)
    reads = read_families(rng, g, 31, unitigs)
    yield p, o, g, unitigs, reads
    p.close()


@pytest.mark.parametrize("k", [16, 31, 63, 127])
def test_summaries_of_every_read_family_in_every_text_mode(k):
    """text modes 0, 1 and 2: in modes 1 and 2 the fast path's reads are summarised from their records (in mode 2 their pairs do not exist); k = 127 leaves no
    records, every read goes through the pair scan.  The call changes neither records nor pairs nor text nor segments"""
    rng = np.random.default_rng(1400 + k)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=max(700, 4 * k))
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    reads = read_families(rng, g, k, unitigs)
    nks = nks_of(reads, k)
    e1 = oracle_pairs(o, reads)
    want = summaries_of(e1, nks)
    want_segs = segments_of(e1, nks)
    found = int((e1[:, 0] != -1).sum())
    # conditions on the expectation itself
    assert (want["n_segments"] == 0).any() and (want["n_segments"] == 1).any() and (want["n_segments"] >= 3).any() and (want_segs[1]["len"] < -1).any()
    assert ((want["n_found"] == 0) & (nks > 0)).any() and (want["span"] > want["n_found"]).any() and ((want["span"] < nks) & (want["n_found"] > 0)).any()
    assert int(want["n_found"].astype(np.int64).sum()) == found
    full = [r for r in reads if len(r) >= k]   # (the text formatter wants a k-mer in every read)
    e2 = oracle_pairs(o, full)
    want_full = summaries_of(e2, nks_of(full, k))
    want_text, at = [], 0
    for r in full:
        want_text.append(format_pairs(e2[at:at + len(r) - k + 1])); at += len(r) - k + 1
    want_text = "".join(want_text).encode()
    for mode in (0, 1, 2):
        b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        assert b.device_read_summaries_ptr() == 0
        got = b.read_summaries()
        assert_summaries(got, want, "k=%d text mode %d" % (k, mode))
        assert b.device_read_summaries_ptr() != 0
        assert int(got["n_found"].astype(np.int64).sum()) == found
        info = b.run_info()
        if k <= 63:
            assert info["fast_path"] and (mode == 0 or b.pipeline_counts()[41] > 0)   # the record path was really taken (modes 1 and 2)
        else:
            assert not info["fast_path"] and b.pipeline_counts()[41] == 0   # every read goes through the scan
        assert_summaries(b.read_summaries(), want, "k=%d text mode %d, a second call" % (k, mode))
        assert_segments(b.segments(), want_segs, "k=%d text mode %d, segments after the summaries" % (k, mode))
        if mode == 2 and info["fast_path"]:
            with pytest.raises(fa.FinitoError):
                b.download()
        else:
            pairs, n = b.download()
            assert n == found and np.array_equal(pairs.astype(np.int64), e1)
        assert_summaries(b.read_summaries(), want, "k=%d text mode %d, after segments and download" % (k, mode))
        b.reload(full)
        with pytest.raises(fa.FinitoError):   # reloaded, not run yet
            b.read_summaries()
        b.run(fa.FIN_MERGED)
        assert b.device_read_summaries_ptr() == 0
        assert_summaries(b.read_summaries(), want_full, "k=%d text mode %d, reads with k-mers" % (k, mode))
        assert b.text() == want_text, "text after the summaries, k=%d mode %d" % (k, mode)
        assert b.download(want_pairs=False)[1] == int((e2[:, 0] != -1).sum())
        assert_summaries(b.read_summaries(), want_full, "k=%d text mode %d, after the text" % (k, mode))
        b.close()
    # an empty batch, a batch of reads without k-mers, a batch of only absent reads
    for rd in ([], ["", "AC"], [random_genome(rng, 200) for _ in range(300)] + ["N" * 200]):
        for mode in (0, 2):
            got = run_summaries(p, rd, mode)
            assert_summaries(got, expected(o, rd, k) if rd else np.zeros(0, fa.READ_SUMMARY_DTYPE), "k=%d %d reads" % (k, len(rd)))
    p.close()


def test_forward_only(set31):
    p, o, g, unitigs, reads = set31
    want = expected(o, reads[:500], 31, fa.FIN_FWD)
    assert (want["n_found"] > 0).sum() > 100 and not np.array_equal(want, expected(o, reads[:500], 31))
    for mode in (0, 2):
        assert_summaries(run_summaries(p, reads[:500], mode, fa.FIN_FWD), want, "forward only, mode %d" % mode)
    got, npos = p.search_reads_summaries(reads[:500], fa.FIN_FWD)
    assert_summaries(got, want, "forward only, host buffers")
    assert npos == int(want["n_found"].astype(np.int64).sum())


def test_a_batch_that_has_not_run_is_refused(set31):
    p, o, g, unitigs, reads = set31
    b = p.batch(reads[:10])
    for call in (b.read_summaries, b.screen):
        with pytest.raises(fa.FinitoError) as e:
            call()
        assert e.value.code == fa.FIN_EINVAL
    assert b.device_read_summaries_ptr() == 0 and b.device_screen_ptr() == (0, 0)
    b.run()
    assert_summaries(b.read_summaries(), expected(o, reads[:10], 31))
    b.close()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("k", [16, 31, 63])
def test_hand_made_records_on_the_device(k, mode):
    """the whole record format (five to eight positions, gaps that touch / overlap / are clamped / cover every slot, both strands, all three kinds in every wave);
    in mode 2 a finished read's pair slots hold garbage, which nobody may read"""
    c = hand_made_case(k)
    p = fa.FinimizerIndex.build(c.unitigs, k).to_device(0)
    b = p.batch(c.reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(c.pairs)
    inject(b, c.recs, c.pairs, mode)
    want = summaries_of(c.pairs, c.nks)
    assert_summaries(b.read_summaries(), want, "k=%d text mode %d" % (k, mode))
    nks = np.asarray(c.nks)
    for scr in SCREENS:
        assert_screen(b.screen(*scr), rule(want, nks, *scr), "k=%d text mode %d screen %s" % (k, mode, scr))
    # other records over the same reads: the summaries and the screen are forgotten and made afresh
    recs2 = np.array(c.recs)
    one = recs2["meta"] >> 16 == 1
    recs2["meta"][one] &= ~np.uint32(0xFF); recs2["Es"][one] = 0; recs2["Es2"][one] = 0   # no position: every slot of a finished read is found
    pairs2 = brute_expand(recs2, c.stream, k)
    want2 = summaries_of(pairs2, c.nks)
    assert not np.array_equal(want2, want) and (want2["n_found"][one] == nks[one]).all()
    inject(b, recs2, pairs2, mode)
    assert b.device_read_summaries_ptr() == 0 and b.device_screen_ptr() == (0, 0)
    assert_screen(b.screen(0, 1000, 0), rule(want2, nks, 0, 1000, 0), "k=%d text mode %d, other records: the screen makes its summaries" % (k, mode))
    assert b.device_read_summaries_ptr() != 0 and all(b.device_screen_ptr())
    assert_summaries(b.read_summaries(), want2, "k=%d text mode %d, other records" % (k, mode))
    b.close()
    p.close()


def test_row_boundaries_of_the_pair_scan():
    """hand-made pairs (set_pairs, text mode 0: every read is scanned) around the scan's rows of 64 slots"""
    k = 31
    rng = np.random.default_rng(1464)
    g = random_genome(rng, 3000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, k, max_len=500), k).to_device(0)
    A = (-1, -1)
    run = lambda u, off, n, step=1: [(u, off + step * i) for i in range(n)]

    def shapes(nk):
        out = [run(0, 100, nk), run(0, 100 + nk, nk, -1), [A] * nk]                        # one segment through the whole read, either direction; nothing
        out.append([(1, 7)] + [A] * (nk - 2) + ([(1, 9)] if nk > 1 else []))                # found at slot 0 and slot nk - 1 only
        for h in (63, 64, 65):
            if nk > h:
                out.append(run(0, 100, h) + run(0, 9000, nk - h))                           # a head exactly at slot h (a jump)
                out.append(run(0, 100, h) + run(2, 100 + h, nk - h))                        # ... (a change of unitig with consecutive offsets)
                out.append(run(0, 100, h) + [A] + run(0, 101 + h, nk - h - 1))              # an absent slot at h
                out.append(run(0, 100, h + 1) + run(0, 100 + h - 1, nk - h - 1, -1))        # a change of direction: the head is slot h + 1
                out.append([A] * h + run(0, 100, nk - h))                                   # the first found slot is h
                out.append(run(0, 100, h) + [A] * (nk - h))                                 # the last found slot is h - 1
        if nk > 67:
            out.append(run(1, 50, 62) + [(2, o) for o in (5, 6, 5, 6, 5)] + run(3, 50, nk - 67))   # 5,6,5,6,5 over slots 62 .. 66
            out.append([A] * 62 + [(2, o) for o in (5, 6, 5, 6, 5)] + [A] * (nk - 67))
        return out

    reads, pairs, nks = [], [], []
    for nk in (1, 63, 64, 65, 127, 128, 129, 200, 5000):
        for s in shapes(nk):
            assert len(s) == nk
            reads.append(random_genome(rng, nk + k - 1)); pairs += s; nks.append(nk)
    pairs = np.array(pairs, dtype=np.int32)
    want = summaries_of(pairs, nks)
    nks = np.array(nks)
    # conditions on the expectation: a segment over 79 rows, the 5,6,5,6,5 rule, span = nk with two found slots
    assert want["longest"].max() == 5000 and ((want["n_found"] == 2) & (want["span"] == nks) & (nks > 2)).sum() >= 7
    assert tuple(want[(nks == 128)][-1].tolist()) == (5, 4, 2, 5) and len(reads) > 150
    b = p.batch(reads); b.text_mode(0); b.run(fa.FIN_MERGED)
    assert b.n_kmers == len(pairs)
    b.read_summaries()
    b.set_pairs(pairs)
    assert b.device_read_summaries_ptr() == 0   # forgotten
    assert_summaries(b.read_summaries(), want, "hand-made pairs")
    assert_segments(b.segments(), segments_of(pairs, nks), "hand-made pairs, segments")
    for scr in SCREENS:
        assert_screen(b.screen(*scr), rule(want, nks, *scr), "hand-made pairs, screen %s" % (scr,))
    b.close()
    p.close()


@pytest.fixture(scope="module")
def screen_set(set31):
    """1 000 reads in random order: present, with 1 % errors, from nowhere, shorter than k -- and what the oracle says of them"""
    p, o, g, unitigs, _ = set31
    rng = np.random.default_rng(1465)
    reads = sample_reads(rng, g, 400, 150, err=0.0, random_frac=0.0) + sample_reads(rng, g, 400, 150, err=0.01, random_frac=0.0)
    reads += [random_genome(rng, 150) for _ in range(120)] + [random_genome(rng, int(rng.integers(0, 31))) for _ in range(80)]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    want = expected(o, reads, 31)
    want.setflags(write=False)
    return reads, want


@pytest.mark.parametrize("n_reads", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_screen(n_reads, set31, screen_set):
    p = set31[0]
    reads, want = screen_set[0][:n_reads], screen_set[1][:n_reads]
    nks = nks_of(reads, 31)
    if n_reads >= 255:   # conditions on the input: every screen keeps some reads and drops some
        for scr in SCREENS[2:]:
            r = rule(want, nks, *scr)
            assert 0 < r.sum() < n_reads, scr
        assert (nks == 0).any() and rule(want, nks, 0, 0, 0).all() and not rule(want, nks, 1, 0, 0)[nks == 0].any()
    b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
    assert b.device_screen_ptr() == (0, 0)
    for scr in SCREENS:
        want_rule = rule(want, nks, *scr)
        got = b.screen(*scr)
        assert_screen(got, want_rule, "%d reads, screen %s" % (n_reads, scr))
        n_pass = fa.C.c_uint64(99)
        err = fa.C.create_string_buffer(512)
        assert fa.lib().fin_batch_screen(b.h, scr[0], scr[1], scr[2], fa.C.byref(n_pass), err, 512) == 0 and n_pass.value == len(got[0]) == int(want_rule.sum())
        assert all(b.device_screen_ptr()) or n_reads == 0
    with pytest.raises(fa.FinitoError) as e:
        b.screen(min_permille=1001)
    assert e.value.code == fa.FIN_EINVAL
    assert_summaries(b.read_summaries(), want, "%d reads: the summaries after the screens" % n_reads)
    b.close()


def sub_batch_reads(nks, max_kmers):
    """the read counts of the sub-batches the host-buffer pipeline cuts (include/finito_amd.h, option max_batch_kmers): a sub-batch takes reads while their
    k-mers fit, and at least one"""
    out, n, kk = [], 0, 0
    for nk in nks:
        if n and kk + nk > max_kmers:
            out.append(n); n, kk = 0, 0
        n += 1; kk += int(nk)
    return out + [n]


def test_host_buffers_in_many_sub_batches(set31):
    p, o, g, unitigs, reads = set31
    nks = nks_of(reads, 31)
    want = expected(o, reads, 31)
    found = int(want["n_found"].astype(np.int64).sum())
    got1, npos1 = p.search_reads_summaries(reads)
    assert_summaries(got1, want, "one batch")
    assert npos1 == found
    pass1 = {scr: p.screen_reads(reads, *scr) for scr in SCREENS}
    for scr in SCREENS:
        assert pass1[scr].dtype == bool and np.array_equal(pass1[scr], rule(want, nks, *scr)), "one batch, screen %s" % (scr,)
    n_kmers = int(nks.sum())
    for sub, depth in ((n_kmers // 6, 3), (20000, 1), (500, 8)):
        cuts = sub_batch_reads(nks, sub)
        assert len(cuts) >= 3 and sum(cuts) == len(reads) and sum(1 for c in cuts[:-1] if c % 64) >= 2   # the cut points do not fall on words of the bitmap
        p.set_option("max_batch_kmers", sub); p.set_option("pipeline_depth", depth)
        try:
            got, npos = p.search_reads_summaries(reads)
            passed = {scr: p.screen_reads(reads, *scr) for scr in SCREENS}
        finally:
            p.set_option("max_batch_kmers", None); p.set_option("pipeline_depth", None)
        assert_summaries(got, got1, "sub-batches of %d k-mers" % sub)
        assert npos == found
        for scr in SCREENS:
            assert np.array_equal(passed[scr], pass1[scr]), "sub-batches of %d k-mers, screen %s" % (sub, scr)
    for rd in ([], ["", "ACG"]):
        got, npos = p.search_reads_summaries(rd)
        assert npos == 0 and len(got) == len(rd) and not got["n_found"].any()
        assert p.screen_reads(rd).tolist() == [False] * len(rd) and p.screen_reads(rd, min_found=0).tolist() == [True] * len(rd)
    with pytest.raises(fa.FinitoError) as e:
        p.screen_reads(reads[:10], min_permille=1001)
    assert e.value.code == fa.FIN_EINVAL
    # the host-side summaries of records + stream are the device's
    recs, stream = p.search_reads_records(reads)
    assert_summaries(fa.records_read_summaries(recs, stream, 31), want, "records_read_summaries of the device's records")


def test_a_withheld_step_has_no_summaries():
    """a step whose overflow list overran (tests/test_segments.py::test_a_withheld_step_has_no_segments' recipe) has no results: FIN_ELIMIT, nothing written"""
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    reads = sample_reads(rng, g, 500, 150)
    L = fa.lib()
    try:
        assert L.fin_set_option(b"lds_deque_limit", 1) == 0 and L.fin_set_option(b"seed_anchors", 0) == 0 and L.fin_set_option(b"debug_ovf_cap", 3) == 0
        for mode in (0, 2):
            b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
            for call in (b.read_summaries, b.screen):
                with pytest.raises(fa.FinitoError) as e:
                    call()
                assert e.value.code == fa.FIN_ELIMIT and "overflow list" in str(e.value)
            assert b.device_read_summaries_ptr() == 0 and b.device_screen_ptr() == (0, 0)
            b.close()
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0
        assert_summaries(run_summaries(p, reads, 2), expected(o, reads, k), "a good step afterwards")
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)
        p.close()
