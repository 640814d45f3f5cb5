"""The per-unitig profile accumulated on the device (include/finito_amd.h: fin_hits, fin_batch_add_hits, fin_search_batch_unitig_counts; fin_hits.hip).

The expected profile is always np.bincount over the ORACLE's pairs of the same reads (oracle/: the reference's algorithm restated on the CPU), never over
this library's own pairs; every comparison is exact equality of all n_unitigs numbers, and total == n_positive == sum(counts)."""
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from finito_amd import synth
from oracle.oracle import OracleIndex, format_pairs
from tests.util import cut_unitigs, defer_family_case, mosaic_read, random_genome, rc, sample_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def profile_of(pairs, n_unitigs):
    u = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)[:, 0]
    return np.bincount(u[u >= 0], minlength=n_unitigs).astype(np.uint64)


def expected(o, reads, n_unitigs, strands=fa.FIN_MERGED):
    if strands == fa.FIN_MERGED:
        return profile_of(o.search_batch(reads, n_threads=8)[0], n_unitigs)
    return profile_of(np.array([x for r in reads for x in o.search(r)[0]], dtype=np.int64).reshape(-1, 2), n_unitigs)   # FinimizerIndex::search on each read


def assert_profile(counts, total, want, what=""):
    assert counts.dtype == np.uint64 and counts.shape == want.shape, what
    bad = np.nonzero(counts != want)[0]
    assert len(bad) == 0, "%s: %d unitigs differ, first %d: got %d, oracle %d" % (what, len(bad), bad[0], counts[bad[0]], want[bad[0]])
    assert total == int(want.sum()), what


def read_families(rng, g, k, unitigs, n=1200):
    """sampled reads with errors and reads from nowhere, mosaics over several unitigs, N's, more than eight substitutions, reads shorter than k"""
    L = max(150, k + 40)
    reads = sample_reads(rng, g, n, L, err=0.01, random_frac=0.08) + [mosaic_read(rng, g, k, 2 * L + 100) for _ in range(n // 6)]
    for i in range(n // 4):
        a = int(rng.integers(0, len(g) - L)); r = list(g[a:a + L])
        if i % 2:
            for _ in range(int(rng.integers(9, 16))): r[int(rng.integers(0, L))] = "ACGT"[int(rng.integers(0, 4))]     # more than eight substitutions
        else:
            for _ in range(int(rng.integers(1, 4))): r[int(rng.integers(0, L))] = "Nn"[int(rng.integers(0, 2))]
        r = "".join(r); reads.append(r if rng.random() < 0.5 else rc(r))
    reads += ["", "ACGT"[: min(4, k - 1)], g[50:50 + k - 1], g[70:70 + k], rc(g[90:90 + k]), g[1000:1300], "A" * L, random_genome(rng, L)]
    reads += list(unitigs[:20]) + [rc(u) for u in unitigs[:20]]
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


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
def test_profile_of_every_read_family_in_every_text_mode(k):
    """text modes 0, 1 and 2: in mode 2 the pairs of the fast path's reads are never written (download still refuses), the profile comes from their records;
    k = 127 leaves no records, every read goes through the pair scan.  The add changes neither records nor pairs: the text afterwards is the oracle's"""
    rng = np.random.default_rng(100 + k)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=max(700, 4 * k))
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    reads = read_families(rng, g, k, unitigs)
    want = expected(o, reads, p.n_unitigs)
    assert want.sum() > 0 and (want > 0).sum() > p.n_unitigs // 2
    full = [r for r in reads if len(r) >= k]   # (the text formatter wants a k-mer in every read)
    e2 = o.search_batch(full, n_threads=8)[0]
    want_full = profile_of(e2, p.n_unitigs)
    want_text, at = [], 0
    for r in full:
        want_text.append(format_pairs(e2[at:at + len(r) - k + 1])); at += len(r) - k + 1
    want_text = "".join(want_text).encode()
    h = p.hits()
    for mode in (0, 1, 2):
        b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        counts, total = h.reset().add(b).download()
        assert_profile(counts, total, want, "k=%d text mode %d" % (k, mode))
        info = b.run_info()
        if mode == 2 and info["fast_path"]:
            with pytest.raises(fa.FinitoError):
                b.download()
        else:
            pairs, npos = b.download()
            assert npos == total and np.array_equal(profile_of(pairs, p.n_unitigs), want)
        b.reload(full); b.run(fa.FIN_MERGED)
        counts, total = h.reset().add(b).download()
        assert_profile(counts, total, want_full, "k=%d text mode %d, reads with k-mers" % (k, mode))
        assert b.text() == want_text, "text after add, k=%d mode %d" % (k, mode)
        assert b.download(want_pairs=False)[1] == total
        b.close()
    # an empty batch, a batch of reads without k-mers, a batch of only absent reads
    for rd in ([], ["", "AC"], [random_genome(rng, 200) for _ in range(300)] + ["N" * 200]):
        b = p.batch(rd); b.text_mode(2); b.run(fa.FIN_MERGED)
        counts, total = h.reset().add(b).download()
        assert_profile(counts, total, expected(o, rd, p.n_unitigs) if rd else np.zeros(p.n_unitigs, np.uint64), "k=%d %d reads" % (k, len(rd)))
        b.close()
    h.close(); p.close()


def test_non_disjoint_sets():
    """identical unitigs, near-duplicates, reverse-complement copies (tests/util.py::defer_family_case): which copy a k-mer is counted in is the reference's choice"""
    rng = np.random.default_rng(555)
    for case in range(10):
        k = (31, 16, 21, 47, 63)[case % 5]
        g, unitigs, reads = defer_family_case(rng, case, k)
        p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
        o = OracleIndex.build(unitigs, k)
        want = expected(o, reads, p.n_unitigs)
        for mode in (2, 0):
            b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
            h = p.hits()
            counts, total = h.add(b).download()
            assert_profile(counts, total, want, "case %d k=%d mode %d" % (case, k, mode))
            h.close(); b.close()
        p.close()


@pytest.mark.parametrize("opts", [{"kernel": 4}, {"kernel": 3}, {"kernel": 2}, {"kernel": 0}, {"fast_path": 0}, {"pp_park": 0}, {"hits_combine": 0}, {"hits_combine": 1},
                                  {"hits_combine": 64}], ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
@pytest.mark.parametrize("strands", [fa.FIN_MERGED, fa.FIN_FWD], ids=["merged", "fwd"])
def test_kernels_strands_and_options(set31, opts, strands):
    p, o, g, unitigs, reads = set31
    rd = reads if strands == fa.FIN_MERGED else reads[:400]
    want = expected(o, rd, p.n_unitigs, strands)
    for name, v in opts.items():
        p.set_option(name, v)
    try:
        for mode in (2, 0):
            b = p.batch(rd); b.text_mode(mode); b.run(strands)
            h = p.hits()
            counts, total = h.add(b).download()
            assert_profile(counts, total, want, "%s mode %d" % (opts, mode))
            h.close(); b.close()
    finally:
        for name in opts:
            p.set_option(name, None)


def test_accumulation_reset_and_independent_accumulators(set31):
    p, o, g, unitigs, reads = set31
    sets = [reads[:500], reads[500:1100], reads[1100:] + reads[:37]]
    wants = [expected(o, s, p.n_unitigs) for s in sets]
    h, h2 = p.hits(), p.hits()
    assert h.device_ptr() and h.device_ptr() != h2.device_ptr()
    b = p.batch(sets[0]); b.text_mode(2)
    for i, s in enumerate(sets):
        if i:
            b.reload(s)
        b.run(fa.FIN_MERGED)
        h.add(b)                              # behind the run, on its stream, no wait in between
        if i == 1:
            h2.add(b)
            assert_profile(*h2.download(), wants[1], "second accumulator")
    counts, total = h.download()
    assert_profile(counts, total, wants[0] + wants[1] + wants[2], "three read sets in one accumulator")
    assert_profile(*h2.download(), wants[1], "second accumulator untouched")
    # adding the same run twice counts it twice; reset gives zeros
    h.add(b)
    assert_profile(*h.download(), wants[0] + wants[1] + 2 * wants[2], "the last run twice")
    counts, total = h.reset().download()
    assert total == 0 and not counts.any()
    assert_profile(*h.add(b).download(), wants[2], "after reset")
    b.close(); h.close(); h2.close()


@pytest.mark.parametrize("n_unitigs", [1, 3])
def test_contention_few_unitigs(n_unitigs):
    """200 000 reads whose hits all go to one or three counters"""
    g = synth.genome(30000, seed=7 + n_unitigs)
    gs = g.tobytes().decode()
    cuts = [0, len(gs)] if n_unitigs == 1 else [0, 9000, 21000, len(gs)]
    unitigs = [gs[max(0, a - 30) if a else 0:b] for a, b in zip(cuts[:-1], cuts[1:])]   # (overlapping by k - 1: every k-mer in one unitig)
    rd = synth.reads(g, 200_000, seed=11)
    p = fa.FinimizerIndex.build(unitigs, 31).to_device(0)
    assert p.n_unitigs == n_unitigs
    o = OracleIndex.build(unitigs, 31)
    want = expected(o, rd.as_tuple(), n_unitigs)
    assert want.sum() > 10_000_000
    for mode, combine in ((2, None), (0, None), (2, 0), (0, 0)):
        p.set_option("hits_combine", combine)
        b = p.batch(rd.as_tuple()); b.text_mode(mode); b.run(fa.FIN_MERGED)
        h = p.hits()
        counts, total = h.add(b).download()
        assert_profile(counts, total, want, "%d unitigs, mode %d, combine %s" % (n_unitigs, mode, combine))
        h.close(); b.close()
    p.set_option("hits_combine", None)
    counts, npos = p.unitig_counts(rd.as_tuple())
    assert_profile(counts, npos, want, "unitig_counts")
    p.close()


def test_many_unitigs():
    g = synth.genome(1_000_000, seed=5)
    u = synth.unitigs(g, 21, max_len=40)
    rd = synth.reads(g, 100_000, seed=6)
    p = fa.FinimizerIndex.build(u.as_tuple(), 21).to_device(0)
    assert p.n_unitigs >= 50_000
    o = OracleIndex.build(u.as_tuple(), 21)
    want = expected(o, rd.as_tuple(), p.n_unitigs)
    assert (want > 0).sum() > 40_000
    for mode in (2, 0):
        b = p.batch(rd.as_tuple()); b.text_mode(mode); b.run(fa.FIN_MERGED)
        h = p.hits()
        counts, total = h.add(b).download()
        assert_profile(counts, total, want, "%d unitigs, mode %d" % (p.n_unitigs, mode))
        h.close(); b.close()
    p.close()


def test_unitig_counts_from_host_buffers_in_many_sub_batches(set31):
    p, o, g, unitigs, reads = set31
    want = expected(o, reads, p.n_unitigs)
    one, npos1 = p.unitig_counts(reads)
    assert_profile(one, npos1, want, "one batch")
    pairs, npos_pairs = p.search_reads(reads)
    assert npos1 == npos_pairs
    for sub, depth in ((3000, 3), (20000, 1), (500, 8)):
        p.set_option("pipeline_kmers", sub); p.set_option("pipeline_depth", depth)
        try:
            many, npos = p.unitig_counts(reads)
        finally:
            p.set_option("pipeline_kmers", None); p.set_option("pipeline_depth", None)
        assert_profile(many, npos, want, "sub-batches of %d k-mers" % sub)
        assert np.array_equal(many, one)
    fwd, nf = p.unitig_counts(reads[:300], fa.FIN_FWD)
    assert_profile(fwd, nf, expected(o, reads[:300], p.n_unitigs, fa.FIN_FWD), "forward only")
    for rd in ([], ["", "ACG"]):
        c, n = p.unitig_counts(rd)
        assert n == 0 and not c.any() and c.shape == (p.n_unitigs,)
    # chunks streamed into one resident accumulator, downloaded once
    h = p.hits()
    h.add_reads(reads[:700]).add_reads(reads[700:]).add_reads([])
    assert_profile(*h.download(), want, "add_reads in two chunks")
    # the host-side counter over records + stream gives the same profile
    recs, stream = p.search_reads_records(reads)
    assert np.array_equal(fa.records_unitig_counts(recs, stream, 31, p.n_unitigs), want)
    h.close()


class _Borrowed:
    """an accumulator handle presented together with an index it does not belong to"""

    def __init__(self, index, hits):
        self.index, self.h, self.L = index, hits.h, hits.L


def test_wrong_pairing_is_refused_and_the_device_stays_usable(set31):
    p, o, g, unitigs, reads = set31
    rng = np.random.default_rng(3)
    other = fa.FinimizerIndex.build(cut_unitigs(rng, random_genome(rng, 5000), 31, max_len=300), 31).to_device(0)
    h, h_other = p.hits(), other.hits()
    b = p.batch(reads[:200])
    with pytest.raises(fa.FinitoError) as e:   # a batch that has not run
        h.add(b)
    assert e.value.code == fa.FIN_EINVAL and "not run" in str(e.value)
    b.text_mode(2); b.run(fa.FIN_MERGED)
    with pytest.raises(fa.FinitoError) as e:   # the accumulator of another index
        h_other.add(b)
    assert e.value.code == fa.FIN_EINVAL and "different" in str(e.value)
    with pytest.raises(fa.FinitoError) as e:   # ... through the host-buffer loop too
        fa.Hits.add_reads(_Borrowed(p, h_other), reads[:10])
    assert e.value.code == fa.FIN_EINVAL and "another index" in str(e.value)
    with pytest.raises(fa.FinitoError):        # no replica on that device
        p.hits(device=63)
    assert not h_other.download()[0].any()
    assert_profile(*h.add(b).download(), expected(o, reads[:200], p.n_unitigs), "after the refusals")
    b.close(); h.close(); h_other.close(); other.close()


def test_a_withheld_step_adds_nothing_and_is_reported_until_the_reset():
    """a step whose overflow list overran (tests/test_unitig_coverage.py::test_a_withheld_step_sets_nothing_and_is_reported_until_the_reset's recipe) has no
    results: the add reads the counter itself, counts nothing and flags the accumulator; fin_hits_download reports FIN_ELIMIT until the reset, after which the
    accumulator is clean and usable"""
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    reads = sample_reads(rng, g, 500, 150)
    want = expected(o, reads, p.n_unitigs)
    L = fa.lib()
    h = p.hits()
    try:
        assert L.fin_set_option(b"lds_deque_limit", 1) == 0 and L.fin_set_option(b"seed_anchors", 0) == 0 and L.fin_set_option(b"debug_ovf_cap", 3) == 0
        for mode in (0, 2):
            b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
            h.add(b)                                   # nobody has looked at the step's overflow counter yet: the kernel does
            with pytest.raises(fa.FinitoError) as e:
                h.download()
            assert e.value.code == fa.FIN_ELIMIT and "overflow list" in str(e.value)
            with pytest.raises(fa.FinitoError) as e:   # ... and keeps saying so
                h.download()
            assert e.value.code == fa.FIN_ELIMIT
            counts, total = h.reset().download()
            assert total == 0 and not counts.any(), "a withheld step was counted (mode %d)" % mode
            with pytest.raises(fa.FinitoError) as e:   # once the host knows (a download looked), the add itself refuses
                b.download(want_pairs=False) if mode == 0 else b.text()
            assert e.value.code == fa.FIN_ELIMIT
            with pytest.raises(fa.FinitoError) as e:
                h.add(b)
            assert e.value.code == fa.FIN_ELIMIT and "overflow list" in str(e.value)
            assert h.download()[1] == 0
            b.close()
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        assert_profile(*h.add(b).download(), want, "a good step after the reset")
        b.close()
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)
        h.close(); p.close()


def test_cli_unitig_counts(tmp_path):
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
    want = expected(o, reads, len(unitigs))
    want_lines = "".join("%d\t%d\n" % (u, int(c)) for u, c in enumerate(want))
    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq"), "--gpus", "1")
    r0 = run(*common, "-o", str(tmp_path / "plain.txt"))
    assert r0.returncode == 0, r0.stderr
    r1 = run(*common, "-o", str(tmp_path / "both.txt"), "--unitig-counts", str(tmp_path / "c1.tsv"))
    assert r1.returncode == 0, r1.stderr
    assert open(tmp_path / "c1.tsv").read() == want_lines
    assert open(tmp_path / "both.txt", "rb").read() == open(tmp_path / "plain.txt", "rb").read() and os.path.getsize(tmp_path / "plain.txt") > 10 * len(reads)
    r2 = run(*common, "-o", str(tmp_path / "none.txt"), "--unitig-counts", str(tmp_path / "c2.tsv"), "--no-text", "1")
    assert r2.returncode == 0, r2.stderr
    assert open(tmp_path / "c2.tsv").read() == want_lines and os.path.getsize(tmp_path / "none.txt") == 0
    r3 = run(*common, "--unitig-counts", str(tmp_path / "c3.tsv"), "--no-text", "1")   # no -o: nothing on stdout either
    assert r3.returncode == 0 and r3.stdout == "" and open(tmp_path / "c3.tsv").read() == want_lines
    found = [ln for ln in r2.stderr.splitlines() if "Total found kmers" in ln]
    assert found and found[0].split()[-1] == str(int(want.sum())) and found == [ln for ln in r0.stderr.splitlines() if "Total found kmers" in ln]
