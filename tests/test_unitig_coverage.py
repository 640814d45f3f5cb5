"""The coverage bitmap accumulated on the device (include/finito_amd.h: fin_cover, fin_batch_add_cover, fin_search_batch_unitig_coverage; fin_cover.hip).

The expected bitmap is always np.unique over the ORACLE's found pairs of the same reads (oracle/: the reference's algorithm restated on the CPU), mapped
through the oracle's unitig ends to bit positions, never this library's own pairs; every comparison is exact equality of the whole bitmap and of all
n_unitigs covered numbers, and total == covered.sum() == popcount(bits)."""
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from finito_amd import synth
from oracle.oracle import OracleIndex, format_pairs
from tests.test_unitig_counts import profile_of, read_families
from tests.util import cut_unitigs, defer_family_case, mosaic_read, random_genome, sample_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


class Want:
    """bits (uint64 words), covered (uint64 per unitig), total = the distinct found places, found = the found pairs"""

    def __init__(self, pairs, ends):
        ends = np.asarray(ends, dtype=np.int64)
        p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        p = p[p[:, 0] >= 0]
        starts = np.concatenate([[0], ends[:-1]])
        g = np.unique(starts[p[:, 0]] + p[:, 1])
        flat = np.zeros(64 * ((int(ends[-1]) + 63) // 64), dtype=np.uint8)
        flat[g] = 1
        self.bits = np.packbits(flat, bitorder="little").view(np.uint64)
        self.covered = np.bincount(np.searchsorted(ends, g, side="right"), minlength=len(ends)).astype(np.uint64)
        self.total, self.found, self.ends = len(g), len(p), ends

    def __or__(self, other):
        w = Want(np.zeros((0, 2), np.int64), self.ends)
        w.bits = self.bits | other.bits
        flat = np.unpackbits(w.bits.view(np.uint8), bitorder="little")
        g = np.nonzero(flat)[0]
        w.covered = np.bincount(np.searchsorted(self.ends, g, side="right"), minlength=len(self.ends)).astype(np.uint64)
        w.total = len(g)
        return w


def oracle_pairs(o, reads, strands=fa.FIN_MERGED):
    if strands == fa.FIN_MERGED:
        return o.search_batch(reads, n_threads=8)[0]
    return np.array([x for r in reads for x in o.search(r)[0]], dtype=np.int64).reshape(-1, 2)   # FinimizerIndex::search on each read


def expected(o, reads, strands=fa.FIN_MERGED):
    return Want(oracle_pairs(o, reads, strands), o.ends())


def assert_cover(got, want, what=""):
    bits, covered, total = got
    assert bits.dtype == np.uint64 and bits.shape == want.bits.shape and covered.dtype == np.uint64 and covered.shape == want.covered.shape, what
    bad = np.nonzero(bits != want.bits)[0]
    assert len(bad) == 0, "%s: %d words differ, first %d: got %016x, oracle %016x" % (what, len(bad), bad[0], bits[bad[0]], want.bits[bad[0]])
    bad = np.nonzero(covered != want.covered)[0]
    assert len(bad) == 0, "%s: covered differs in %d unitigs, first %d: got %d, oracle %d" % (what, len(bad), bad[0], covered[bad[0]], want.covered[bad[0]])
    assert total == want.total == int(covered.sum()) == int(np.unpackbits(bits.view(np.uint8)).sum()), what


def assert_inputs_show_something(want, n_kmers, k):
    """conditions on the inputs, checked on the oracle's expectation: some k-mer is hit more than once, some never, more than half the unitigs are touched, one
    unitig is covered end to end"""
    assert 0 < want.total < want.found and want.total < n_kmers
    assert (want.covered > 0).sum() > len(want.covered) // 2
    lens = np.diff(np.concatenate([[0], want.ends]))
    assert (want.covered == (lens - k + 1).astype(np.uint64)).any()


@pytest.fixture(scope="module")
def set31():
    rng = np.random.default_rng(20260)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, 31, max_len=700)
    p = fa.FinimizerIndex.build(unitigs, 31).to_device(0)
    o = OracleIndex.build(unitigs, 31)
    reads = read_families(rng, g, 31, unitigs)
    yield p, o, g, unitigs, reads
    p.close()


@pytest.mark.parametrize("k", [16, 31, 63, 127])
def test_bitmap_of_every_read_family_in_every_text_mode(k):
    """text modes 0, 1 and 2: in mode 2 the bits of the fast path's reads come from their records; k = 127 leaves no records, every read goes through the pair
    scan.  The add changes neither records nor pairs: text and pairs afterwards are the oracle's.  No bit in the last k - 1 positions of any unitig"""
    rng = np.random.default_rng(100 + k)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=max(700, 4 * k))
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    assert np.array_equal(p.export(fa.X_ENDS), o.ends())
    reads = read_families(rng, g, k, unitigs)
    e1 = oracle_pairs(o, reads)
    want = Want(e1, o.ends())
    assert_inputs_show_something(want, p.n_kmers, k)
    full = [r for r in reads if len(r) >= k]   # (the text formatter wants a k-mer in every read)
    e2 = oracle_pairs(o, full)
    want_full = Want(e2, o.ends())
    want_text, at = [], 0
    for r in full:
        want_text.append(format_pairs(e2[at:at + len(r) - k + 1])); at += len(r) - k + 1
    want_text = "".join(want_text).encode()
    tail = np.zeros(64 * len(want.bits), dtype=bool)   # the last k - 1 positions of every unitig
    for e in o.ends():
        tail[e - (k - 1):e] = True
    c = p.cover()
    assert c.device_ptr()
    for mode in (0, 1, 2):
        b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        got = c.reset().add(b).download()
        assert_cover(got, want, "k=%d text mode %d" % (k, mode))
        assert not np.unpackbits(got[0].view(np.uint8), bitorder="little")[tail].any()
        info = b.run_info()
        if mode == 2 and info["fast_path"]:
            with pytest.raises(fa.FinitoError):
                b.download()
        else:
            pairs, npos = b.download()
            assert npos == want.found and np.array_equal(pairs.astype(np.int64), e1)
        b.reload(full); b.run(fa.FIN_MERGED)
        assert_cover(c.reset().add(b).download(), want_full, "k=%d text mode %d, reads with k-mers" % (k, mode))
        assert b.text() == want_text, "text after add, k=%d mode %d" % (k, mode)
        assert b.download(want_pairs=False)[1] == want_full.found
        b.close()
    # an empty batch, a batch of reads without k-mers, a batch of only absent reads
    for rd in ([], ["", "AC"], [random_genome(rng, 200) for _ in range(300)] + ["N" * 200]):
        b = p.batch(rd); b.text_mode(2); b.run(fa.FIN_MERGED)
        assert_cover(c.reset().add(b).download(), expected(o, rd) if rd else Want(np.zeros((0, 2)), o.ends()), "k=%d %d reads" % (k, len(rd)))
        b.close()
    c.close(); p.close()


def test_non_disjoint_sets():
    """identical unitigs, near-duplicates, reverse-complement copies (tests/util.py::defer_family_case): only the copy the reference reports is set"""
    rng = np.random.default_rng(555)
    for case in range(10):
        k = (31, 16, 21, 47, 63)[case % 5]
        g, unitigs, reads = defer_family_case(rng, case, k)
        p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
        o = OracleIndex.build(unitigs, k)
        want = expected(o, reads)
        assert want.total > 0
        for mode in (2, 0):
            b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
            c = p.cover()
            assert_cover(c.add(b).download(), want, "case %d k=%d mode %d" % (case, k, mode))
            c.close(); b.close()
        p.close()


@pytest.mark.parametrize("opts", [{"kernel": 4}, {"kernel": 3}, {"kernel": 2}, {"kernel": 0}, {"fast_path": 0}, {"pp_park": 0}, {"cover_probe": 0}, {"cover_probe": 1}],
                         ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
@pytest.mark.parametrize("strands", [fa.FIN_MERGED, fa.FIN_FWD], ids=["merged", "fwd"])
def test_kernels_strands_and_options(set31, opts, strands):
    p, o, g, unitigs, reads = set31
    rd = reads if strands == fa.FIN_MERGED else reads[:400]
    want = expected(o, rd, strands)
    assert want.total > 0
    for name, v in opts.items():
        p.set_option(name, v)
    try:
        for mode in (2, 0):
            b = p.batch(rd); b.text_mode(mode); b.run(strands)
            c = p.cover()
            assert_cover(c.add(b).add(b).download(), want, "%s mode %d" % (opts, mode))   # (the second add finds every word full: the probe's other branch)
            c.close(); b.close()
    finally:
        for name in opts:
            p.set_option(name, None)


def test_idempotence_accumulation_reset_and_independent_accumulators(set31):
    p, o, g, unitigs, reads = set31
    sets = [reads[:500], reads[500:1100], reads[1100:] + reads[:37]]
    wants = [expected(o, s) for s in sets]
    c, c2 = p.cover(), p.cover()
    assert c.device_ptr() and c.device_ptr() != c2.device_ptr()
    b = p.batch(sets[0]); b.text_mode(2)
    for i, s in enumerate(sets):
        if i:
            b.reload(s)
        b.run(fa.FIN_MERGED)
        c.add(b)                              # behind the run, on its stream, no wait in between
        if i == 1:
            c2.add(b)
            assert_cover(c2.download(), wants[1], "second accumulator")
    union = wants[0] | wants[1] | wants[2]
    assert union.total > max(w.total for w in wants)
    assert_cover(c.download(), union, "three read sets in one accumulator")
    assert_cover(c2.download(), wants[1], "second accumulator untouched")
    # adding the same run twice changes nothing; reset gives zeros
    c.add(b)
    assert_cover(c.download(), union, "the last run twice")
    bits, covered, total = c.reset().download()
    assert total == 0 and not bits.any() and not covered.any()
    assert_cover(c.add(b).download(), wants[2], "after reset")
    b.close(); c.close(); c2.close()


def test_hits_and_cover_from_the_same_run(set31):
    p, o, g, unitigs, reads = set31
    pairs = oracle_pairs(o, reads)
    want = Want(pairs, o.ends())
    for mode in (2, 0):
        b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        h, c = p.hits(), p.cover()
        h.add(b); c.add(b); h.add(b)
        assert_cover(c.download(), want, "cover beside hits, mode %d" % mode)
        counts, total = h.download()
        assert np.array_equal(counts, 2 * profile_of(pairs, p.n_unitigs)) and total == 2 * want.found
        h.close(); c.close(); b.close()


@pytest.mark.parametrize("n_unitigs", [1, 3])
def test_contention_few_unitigs(n_unitigs):
    """200 000 reads on 30 000 bases: every word is contended and everything saturates; one unitig of 30 000 bases for the popcount"""
    g = synth.genome(30000, seed=7 + n_unitigs)
    gs = g.tobytes().decode()
    cuts = [0, len(gs)] if n_unitigs == 1 else [0, 9000, 21000, len(gs)]
    unitigs = [gs[max(0, a - 30) if a else 0:b] for a, b in zip(cuts[:-1], cuts[1:])]   # (overlapping by k - 1: every k-mer in one unitig)
    rd = synth.reads(g, 200_000, seed=11)
    p = fa.FinimizerIndex.build(unitigs, 31).to_device(0)
    assert p.n_unitigs == n_unitigs
    o = OracleIndex.build(unitigs, 31)
    want = expected(o, rd.as_tuple())
    assert want.found > 10_000_000 and want.total > 0.9 * p.n_kmers
    for mode, probe in ((2, 1), (0, 1), (2, 0), (0, 0)):
        p.set_option("cover_probe", probe)
        b = p.batch(rd.as_tuple()); b.text_mode(mode); b.run(fa.FIN_MERGED)
        c = p.cover()
        assert_cover(c.add(b).download(), want, "%d unitigs, mode %d, probe %d" % (n_unitigs, mode, probe))
        c.close(); b.close()
    p.set_option("cover_probe", None)
    covered, npos = p.unitig_coverage(rd.as_tuple())
    assert np.array_equal(covered, want.covered) and npos == want.found
    p.close()


def test_many_unitigs():
    """more than 5e4 unitigs of at most 40 bases at k = 21: several unitigs share one bitmap word"""
    g = synth.genome(1_000_000, seed=5)
    u = synth.unitigs(g, 21, max_len=40)
    rd = synth.reads(g, 100_000, seed=6)
    p = fa.FinimizerIndex.build(u.as_tuple(), 21).to_device(0)
    assert p.n_unitigs >= 50_000
    o = OracleIndex.build(u.as_tuple(), 21)
    assert int(np.diff(np.concatenate([[0], o.ends()])).max()) <= 40
    want = expected(o, rd.as_tuple())
    assert (want.covered > 0).sum() > 40_000 and want.total < want.found
    for mode in (2, 0):
        b = p.batch(rd.as_tuple()); b.text_mode(mode); b.run(fa.FIN_MERGED)
        c = p.cover()
        assert_cover(c.add(b).download(), want, "%d unitigs, mode %d" % (p.n_unitigs, mode))
        c.close(); b.close()
    p.close()


def test_coverage_from_host_buffers_in_many_sub_batches(set31):
    p, o, g, unitigs, reads = set31
    want = expected(o, reads)
    one, npos1 = p.unitig_coverage(reads)
    assert np.array_equal(one, want.covered) and npos1 == want.found
    for sub, depth in ((3000, 3), (20000, 1), (500, 8)):
        p.set_option("pipeline_kmers", sub); p.set_option("pipeline_depth", depth)
        try:
            many, npos = p.unitig_coverage(reads)
            c = p.cover()
            got = c.add_reads(reads).download()
            c.close()
        finally:
            p.set_option("pipeline_kmers", None); p.set_option("pipeline_depth", None)
        assert np.array_equal(many, want.covered) and npos == want.found, "sub-batches of %d k-mers" % sub
        assert_cover(got, want, "add_reads in sub-batches of %d k-mers" % sub)
    fwd, nf = p.unitig_coverage(reads[:300], fa.FIN_FWD)
    wf = expected(o, reads[:300], fa.FIN_FWD)
    assert np.array_equal(fwd, wf.covered) and nf == wf.found
    for rd in ([], ["", "ACG"]):
        cov, n = p.unitig_coverage(rd)
        assert n == 0 and not cov.any() and cov.shape == (p.n_unitigs,)
    # chunks streamed into one resident accumulator, downloaded once
    c = p.cover()
    c.add_reads(reads[:700]).add_reads(reads[700:]).add_reads([])
    assert_cover(c.download(), want, "add_reads in two chunks")
    # the host-side bitmap over records + stream is the device's
    recs, stream = p.search_reads_records(reads)
    assert np.array_equal(fa.records_cover(recs, stream, 31, p.export(fa.X_ENDS)), c.download()[0])
    assert np.array_equal(fa.records_cover(recs, stream, 31, o.ends()), want.bits)
    c.close()


class _Borrowed:
    """an accumulator handle presented together with an index it does not belong to"""

    def __init__(self, index, cover):
        self.index, self.h, self.L = index, cover.h, cover.L


def test_wrong_pairing_is_refused_and_the_device_stays_usable(set31):
    p, o, g, unitigs, reads = set31
    rng = np.random.default_rng(3)
    other = fa.FinimizerIndex.build(cut_unitigs(rng, random_genome(rng, 5000), 31, max_len=300), 31).to_device(0)
    c, c_other = p.cover(), other.cover()
    b = p.batch(reads[:200])
    with pytest.raises(fa.FinitoError) as e:   # a batch that has not run
        c.add(b)
    assert e.value.code == fa.FIN_EINVAL and "not run" in str(e.value)
    b.text_mode(2); b.run(fa.FIN_MERGED)
    with pytest.raises(fa.FinitoError) as e:   # the accumulator of another index
        c_other.add(b)
    assert e.value.code == fa.FIN_EINVAL and "different" in str(e.value)
    with pytest.raises(fa.FinitoError) as e:   # ... through the host-buffer loop too
        fa.Cover.add_reads(_Borrowed(p, c_other), reads[:10])
    assert e.value.code == fa.FIN_EINVAL and "another index" in str(e.value)
    with pytest.raises(fa.FinitoError):        # no replica on that device
        p.cover(device=63)
    assert not c_other.download()[0].any()
    assert_cover(c.add(b).download(), expected(o, reads[:200]), "after the refusals")
    b.close(); c.close(); c_other.close(); other.close()


def test_a_withheld_step_sets_nothing_and_is_reported_until_the_reset():
    """a step whose overflow list overran (tests/test_search_gpu.py::test_deque_overflow_path's recipe) has no results: the add reads the counter itself, sets
    nothing and flags the accumulator; fin_cover_download reports FIN_ELIMIT until the reset, after which the accumulator is clean and usable"""
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    reads = sample_reads(rng, g, 500, 150)
    want = expected(o, reads)
    L = fa.lib()
    c = p.cover()
    try:
        assert L.fin_set_option(b"lds_deque_limit", 1) == 0 and L.fin_set_option(b"seed_anchors", 0) == 0 and L.fin_set_option(b"debug_ovf_cap", 3) == 0
        for mode in (0, 2):
            b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
            c.add(b)                                   # nobody has looked at the step's overflow counter yet: the kernel does
            with pytest.raises(fa.FinitoError) as e:
                c.download()
            assert e.value.code == fa.FIN_ELIMIT and "overflow list" in str(e.value)
            with pytest.raises(fa.FinitoError) as e:   # ... and keeps saying so
                c.download()
            assert e.value.code == fa.FIN_ELIMIT
            bits, covered, total = c.reset().download()
            assert total == 0 and not bits.any() and not covered.any(), "a withheld step set bits (mode %d)" % mode
            with pytest.raises(fa.FinitoError) as e:   # once the host knows (a download looked), the add itself refuses
                b.download(want_pairs=False) if mode == 0 else b.text()
            assert e.value.code == fa.FIN_ELIMIT
            with pytest.raises(fa.FinitoError) as e:
                c.add(b)
            assert e.value.code == fa.FIN_ELIMIT
            b.close()
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        assert_cover(c.add(b).download(), want, "a good step after the reset")
        b.close()
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)
        c.close(); p.close()


def test_places_outside_the_index_are_skipped_and_reported(set31):
    """hand-made pairs (fin_batch_set_pairs; the flat scan): ascending and descending runs, runs across a word boundary and across rows of 64 slots, a direction
    change inside a run -- and a unitig number the index does not have, a position beyond the text: skipped, everything else set, FIN_EINVAL until the reset"""
    p, o, g, unitigs, reads = set31
    ends = o.ends()
    lens = np.diff(np.concatenate([[0], ends]))
    rng = np.random.default_rng(77)
    rd = [random_genome(rng, 150) for _ in range(40)]
    b = p.batch(rd); b.text_mode(0); b.run(fa.FIN_MERGED)
    n = b.n_kmers
    u_long = int(np.argmax(lens)); L_ = int(lens[u_long]) - 31 + 1
    assert L_ > 300
    good = np.full((n, 2), -1, dtype=np.int64)
    at = 3
    for offs in (range(0, 200), range(L_ - 1, L_ - 1 - 150, -1), [10, 11, 12, 11, 10, 9, 10], [5], range(250, 260)):
        for x in offs:
            good[at] = (u_long, x); at += 1
        at += int(rng.integers(0, 3))
    u2 = (u_long + 1) % len(ends)
    for x in range(int(lens[u2]) - 31, -1, -1):   # a whole unitig, descending
        good[at] = (u2, x); at += 1
    assert at < n - 10
    c = p.cover()
    for probe in (0, 1):
        p.set_option("cover_probe", probe)
        try:
            b.set_pairs(good)
            assert_cover(c.reset().add(b).add(b).download(), Want(good, ends), "hand-made runs, probe %d" % probe)
            bad = good.copy()
            bad[at + 2] = (p.n_unitigs + 5, 0)                                            # a unitig the index does not have
            bad[at + 4] = (p.n_unitigs - 1, int(lens[-1]))                                # the first position beyond the text
            bad[at + 6] = (p.n_unitigs - 1, int(lens[-1]) + 100000)
            b.set_pairs(bad)
            c.reset().add(b)
            with pytest.raises(fa.FinitoError) as e:
                c.download()
            assert e.value.code == fa.FIN_EINVAL and "outside the index" in str(e.value)
            b.set_pairs(good)
            assert_cover(c.reset().add(b).download(), Want(good, ends), "after the reset, probe %d" % probe)
        finally:
            p.set_option("cover_probe", None)
    c.close(); b.close()


def test_cli_unitig_coverage(tmp_path):
    rng = np.random.default_rng(99)
    g = random_genome(rng, 30000)
    unitigs = cut_unitigs(rng, g, 31, max_len=500)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    reads = [r for r in sample_reads(rng, g, 3000, 150, err=0.01, random_frac=0.05) + [mosaic_read(rng, g, 31, 300) for _ in range(300)] if len(r) >= 1]
    with open(tmp_path / "q.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    run = lambda *a: subprocess.run([BIN, *a], capture_output=True, text=True)
    r = run("build-fmin", "-o", str(tmp_path / "idx"), "-u", str(tmp_path / "u.fna"), "-k", "31")
    assert r.returncode == 0, r.stderr
    o = OracleIndex.build(unitigs, 31)
    pairs = oracle_pairs(o, reads)
    want = Want(pairs, o.ends())
    lens = np.diff(np.concatenate([[0], o.ends()]))
    want_lines = "".join("%d\t%d\t%d\n" % (u, lens[u] - 31 + 1, int(c)) for u, c in enumerate(want.covered))
    want_counts = "".join("%d\t%d\n" % (u, int(c)) for u, c in enumerate(profile_of(pairs, len(unitigs))))
    assert 0 < want.total < want.found
    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq"), "--gpus", "1")
    r0 = run(*common, "-o", str(tmp_path / "plain.txt"))
    assert r0.returncode == 0, r0.stderr
    r1 = run(*common, "-o", str(tmp_path / "both.txt"), "--unitig-coverage", str(tmp_path / "c1.tsv"))
    assert r1.returncode == 0, r1.stderr
    assert open(tmp_path / "c1.tsv").read() == want_lines
    assert open(tmp_path / "both.txt", "rb").read() == open(tmp_path / "plain.txt", "rb").read() and os.path.getsize(tmp_path / "plain.txt") > 10 * len(reads)
    r2 = run(*common, "-o", str(tmp_path / "all.txt"), "--unitig-coverage", str(tmp_path / "c2.tsv"), "--unitig-counts", str(tmp_path / "n2.tsv"))
    assert r2.returncode == 0, r2.stderr
    assert open(tmp_path / "c2.tsv").read() == want_lines and open(tmp_path / "n2.tsv").read() == want_counts
    assert open(tmp_path / "all.txt", "rb").read() == open(tmp_path / "plain.txt", "rb").read()
    r3 = run(*common, "--unitig-coverage", str(tmp_path / "c3.tsv"), "--no-text", "1")   # no -o: nothing on stdout either
    assert r3.returncode == 0 and r3.stdout == "" and open(tmp_path / "c3.tsv").read() == want_lines
    r4 = run(*common, "--unitig-coverage", str(tmp_path / "c4.tsv"))                      # alone: the text goes to stdout
    assert r4.returncode == 0 and open(tmp_path / "c4.tsv").read() == want_lines and r4.stdout.encode() == open(tmp_path / "plain.txt", "rb").read()
    found = [ln for ln in r3.stderr.splitlines() if "Total found kmers" in ln]
    assert found and found[0].split()[-1] == str(want.found) and found == [ln for ln in r0.stderr.splitlines() if "Total found kmers" in ln]
