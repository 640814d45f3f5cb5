"""Results as segments, on the device (include/finito_amd.h: fin_batch_segments, fin_search_batch_segments; fin_segments.hip).  The expectation is always the
definition written in numpy (tests/test_segments_host.py::segments_of) over the ORACLE's pairs."""
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from oracle.oracle import OracleIndex, format_pairs
from tests.test_segments_host import assert_segments, segments_of
from tests.test_unitig_counts import read_families
from tests.util import cut_unitigs, defer_family_case, mosaic_read, random_genome, rc, sample_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "finito_amd", "finito")


def oracle_pairs(o, reads, strands=fa.FIN_MERGED):
    if strands == fa.FIN_MERGED:
        return o.search_batch(reads, n_threads=8)[0]
    return np.array([x for r in reads for x in o.search(r)[0]], dtype=np.int64).reshape(-1, 2)   # FinimizerIndex::search on each read


def nks_of(reads, k):
    return np.array([max(0, len(r) - k + 1) for r in reads], dtype=np.int64)


def expected(o, reads, k, strands=fa.FIN_MERGED):
    return segments_of(oracle_pairs(o, reads, strands), nks_of(reads, k))


def run_segments(p, reads, mode=0, strands=fa.FIN_MERGED):
    b = p.batch(reads); b.text_mode(mode); b.run(strands)
    got = b.segments()
    b.close()
    return got


@pytest.fixture(scope="module")
def set31():
    rng = np.random.default_rng(20310)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, 31, max_len=700)
    p = fa.FinimizerIndex.build(unitigs, 31).to_device(0)
    o = OracleIndex.build(unitigs, 31)
    reads = read_families(rng, g, 31, unitigs)
    yield p, o, g, unitigs, reads
    p.close()


@pytest.mark.parametrize("k", [16, 31, 63, 127])
def test_segments_of_every_read_family_in_every_text_mode(k):
    """text modes 0, 1 and 2: in modes 1 and 2 the fast path's reads are segmented from their records (in mode 2 their pairs do not exist); k = 127 leaves no
    records, every read goes through the pair scan.  The call changes neither records nor pairs nor text"""
    rng = np.random.default_rng(300 + k)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=max(700, 4 * k))
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    reads = read_families(rng, g, k, unitigs)
    e1 = oracle_pairs(o, reads)
    want = segments_of(e1, nks_of(reads, k))
    per_read = np.diff(want[0].astype(np.int64))
    assert (want[1]["len"] < -1).any() and (want[1]["len"] > 1).any() and (want[1]["len"] == 1).any() and (per_read >= 3).any() and (per_read == 0).any()
    full = [r for r in reads if len(r) >= k]   # (the text formatter wants a k-mer in every read)
    e2 = oracle_pairs(o, full)
    want_full = segments_of(e2, nks_of(full, k))
    want_text, at = [], 0
    for r in full:
        want_text.append(format_pairs(e2[at:at + len(r) - k + 1])); at += len(r) - k + 1
    want_text = "".join(want_text).encode()
    for mode in (0, 1, 2):
        b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        assert b.device_segments_ptr() == (0, 0)
        got = b.segments()
        assert_segments(got, want, "k=%d text mode %d" % (k, mode))
        assert all(b.device_segments_ptr())
        back, npos = fa.expand_segments(got[0], got[1], nks_of(reads, k))
        assert np.array_equal(back.astype(np.int64), e1) and npos == int((e1[:, 0] != -1).sum())
        info = b.run_info()
        if k <= 63:
            assert info["fast_path"] and b.pipeline_counts()[41] > 0   # the record path was really taken (modes 1 and 2)
        else:
            assert not info["fast_path"] and b.pipeline_counts()[41] == 0   # every read goes through the scan
        if mode == 2 and info["fast_path"]:
            with pytest.raises(fa.FinitoError):
                b.download()
        else:
            pairs, n = b.download()
            assert n == int((e1[:, 0] != -1).sum()) and np.array_equal(pairs.astype(np.int64), e1)
        assert_segments(b.segments(), want, "k=%d text mode %d, a second call" % (k, mode))
        b.reload(full); b.run(fa.FIN_MERGED)
        assert_segments(b.segments(), want_full, "k=%d text mode %d, reads with k-mers" % (k, mode))
        assert b.text() == want_text, "text after segments, k=%d mode %d" % (k, mode)
        assert b.download(want_pairs=False)[1] == int((e2[:, 0] != -1).sum())
        assert_segments(b.segments(), want_full, "k=%d text mode %d, after the text" % (k, mode))
        b.close()
    # an empty batch, a batch of reads without k-mers, a batch of only absent reads
    for rd in ([], ["", "AC"], [random_genome(rng, 200) for _ in range(300)] + ["N" * 200]):
        for mode in (0, 2):
            got = run_segments(p, rd, mode)
            assert_segments(got, expected(o, rd, k) if rd else (np.zeros(1, np.uint64), np.zeros(0, fa.SEGMENT_DTYPE)), "k=%d %d reads" % (k, len(rd)))
    p.close()


def test_forward_only(set31):
    p, o, g, unitigs, reads = set31
    want = expected(o, reads[:500], 31, fa.FIN_FWD)
    assert len(want[1]) > 100
    for mode in (0, 2):
        assert_segments(run_segments(p, reads[:500], mode, fa.FIN_FWD), want, "forward only, mode %d" % mode)


def test_a_batch_that_has_not_run_is_refused(set31):
    p, o, g, unitigs, reads = set31
    b = p.batch(reads[:10])
    with pytest.raises(fa.FinitoError) as e:
        b.segments()
    assert e.value.code == fa.FIN_EINVAL
    b.run()
    assert_segments(b.segments(), expected(o, reads[:10], 31))
    b.close()


def test_non_disjoint_sets():
    """identical unitigs, near-duplicates, reverse-complement copies (tests/util.py::defer_family_case), and the duplicated / reverse-complemented set of
    tests/test_records.py"""
    from tests.test_search_gpu import _fast_path_reads
    rng = np.random.default_rng(556)
    for case in range(10):
        k = (31, 16, 21, 47, 63)[case % 5]
        g, unitigs, reads = defer_family_case(rng, case, k)
        p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
        o = OracleIndex.build(unitigs, k)
        want = expected(o, reads, k)
        assert len(want[1]) > 0
        for mode in (2, 0):
            assert_segments(run_segments(p, reads, mode), want, "case %d k=%d mode %d" % (case, k, mode))
        p.close()
    k = 31
    g = random_genome(rng, 40000)
    for _ in range(5):
        a = int(rng.integers(0, len(g) - 300)); n = int(rng.integers(k + 3, 300)); at = int(rng.integers(0, len(g)))
        g = g[:at] + g[a:a + n] + g[at:]
    unitigs = cut_unitigs(rng, g, k, max_len=900, flip=False) + [rc(g[a:a + 200]) for a in (1000, 7000)]
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    reads = _fast_path_reads(rng, g, k, unitigs) + ["", "ACGT", g[100:100 + k - 1]]
    want = expected(o, reads, k)
    for mode in (2, 1, 0):
        assert_segments(run_segments(p, reads, mode), want, "duplicated stretches, mode %d" % mode)
    so, sg, npos = p.search_reads_segments(reads)
    assert_segments((so, sg), want, "duplicated stretches, host buffers")
    p.close()


def test_periodic_and_homopolymer_reads():
    """a period-2 read over a unitig that holds ACAC..., a homopolymer read over a unitig that holds AAAA...: the same k-mer again and again -- whatever places the
    reference reports, the segments are the rule's"""
    rng = np.random.default_rng(557)
    for k in (16, 31):
        g = random_genome(rng, 6000)
        unitigs = cut_unitigs(rng, g, k, max_len=500) + [random_genome(rng, 40) + "AC" * (k + 20) + random_genome(rng, 40), random_genome(rng, 40) + "A" * (2 * k + 9) + random_genome(rng, 40)]
        p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
        o = OracleIndex.build(unitigs, k)
        reads = ["AC" * (k + 10), "CA" * (k + 10), "A" * (2 * k + 5), "T" * (2 * k + 5), "GT" * (k + 10), unitigs[-2], rc(unitigs[-2]), unitigs[-1], rc(unitigs[-1])]
        reads += sample_reads(rng, g, 100, 150, err=0.01, random_frac=0.05)
        e = oracle_pairs(o, reads)
        want = segments_of(e, nks_of(reads, k))
        per_read = np.diff(want[0].astype(np.int64))
        nks = nks_of(reads, k)
        assert (e[:nks[0], 0] != -1).all() and per_read[0] >= nks[0] // 2       # the period-2 read: found everywhere, (almost) no two slots join
        assert per_read[2] == nks[2] and (e[nks[:2].sum():nks[:3].sum(), 0] != -1).all()   # the homopolymer: a repeated identical pair, nk segments of one slot
        for mode in (0, 1, 2):
            assert_segments(run_segments(p, reads, mode), want, "k=%d mode %d" % (k, mode))
        p.close()


def test_a_long_read_across_many_unitigs_and_a_segment_across_many_rows():
    rng = np.random.default_rng(558)
    k = 31
    g = random_genome(rng, 60000)
    unitigs = cut_unitigs(rng, g[:30000], k, max_len=700) + cut_unitigs(rng, g[30000 - k + 1:], k, max_len=9000)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    def with_errors(s, n):
        s = list(s)
        for _ in range(n):
            s[int(rng.integers(0, len(s)))] = "ACGT"[int(rng.integers(0, 4))]
        return "".join(s)
    reads = [g[5000:15000], rc(g[12000:22000]), with_errors(g[3000:13000], 12), g[31000:41000], rc(g[45000:55000]), with_errors(g[25000:35000], 5),
             g[100:100 + 64 + k - 1], g[200:200 + 65 + k - 1], g[300:300 + 63 + k - 1], g[31000:31000 + 128 + k - 1], g[31000:31000 + 129 + k - 1]]
    reads += sample_reads(rng, g, 200, 150, err=0.01, random_frac=0.05)
    want = expected(o, reads, k)
    per_read = np.diff(want[0].astype(np.int64))
    n_abs = np.abs(want[1]["len"].astype(np.int64))
    assert per_read[0] > 10 and n_abs.max() > 4096 and (n_abs[: int(want[0][6])] > 64).sum() > 20
    assert (want[1]["len"] < -64).any() and (want[1]["len"] > 64).any()
    for mode in (0, 2):
        got = run_segments(p, reads, mode)
        assert_segments(got, want, "mode %d" % mode)
    so, sg, npos = p.search_reads_segments(reads)
    assert_segments((so, sg), want, "host buffers")
    assert npos == int(n_abs.sum())
    p.close()


def test_segments_from_host_buffers_in_many_sub_batches(set31):
    p, o, g, unitigs, reads = set31
    e = oracle_pairs(o, reads)
    want = segments_of(e, nks_of(reads, 31))
    found = int((e[:, 0] != -1).sum())
    so1, sg1, npos1 = p.search_reads_segments(reads)
    assert_segments((so1, sg1), want, "one batch")
    assert npos1 == found and so1[-1] == len(sg1)
    n_kmers = int(nks_of(reads, 31).sum())
    for sub, depth in ((n_kmers // 6, 3), (20000, 1), (500, 8)):
        assert n_kmers // sub >= 5
        p.set_option("max_batch_kmers", sub); p.set_option("pipeline_depth", depth)
        try:
            so, sg, npos = p.search_reads_segments(reads)
        finally:
            p.set_option("max_batch_kmers", None); p.set_option("pipeline_depth", None)
        assert_segments((so, sg), (so1, sg1), "sub-batches of %d k-mers" % sub)
        assert npos == found
    wf = expected(o, reads[:300], 31, fa.FIN_FWD)
    so, sg, npos = p.search_reads_segments(reads[:300], fa.FIN_FWD)
    assert_segments((so, sg), wf, "forward only")
    assert npos == int(np.abs(wf[1]["len"].astype(np.int64)).sum())
    for rd in ([], ["", "ACG"]):
        so, sg, npos = p.search_reads_segments(rd)
        assert npos == 0 and len(sg) == 0 and so.tolist() == [0] * (len(rd) + 1)
    # the host-side segmentation of records + stream is the device's
    recs, stream = p.search_reads_records(reads)
    assert_segments(fa.records_segments(recs, stream, 31), want, "records_segments of the device's records")
    # room for one segment too few
    L = fa.lib()
    import ctypes as C
    bases, offsets = fa.flatten(reads)
    so = np.zeros(len(reads) + 1, dtype=np.uint64); sg = np.zeros(len(sg1), dtype=fa.SEGMENT_DTYPE)
    err = C.create_string_buffer(512)
    rc_ = L.fin_search_batch_segments(p.h, bases.ctypes.data_as(C.c_char_p), offsets.ctypes.data_as(C.POINTER(C.c_uint64)), len(reads), fa.FIN_MERGED,
                                      so.ctypes.data_as(C.POINTER(C.c_uint64)), sg.ctypes.data_as(C.c_void_p), len(sg1) - 1, None, None, err, 512)
    assert rc_ == fa.FIN_ELIMIT
    rc_ = L.fin_search_batch_segments(p.h, bases.ctypes.data_as(C.c_char_p), offsets.ctypes.data_as(C.POINTER(C.c_uint64)), len(reads), fa.FIN_MERGED,
                                      so.ctypes.data_as(C.POINTER(C.c_uint64)), sg.ctypes.data_as(C.c_void_p), len(sg1), None, None, err, 512)
    assert rc_ == fa.FIN_OK
    assert_segments((so, sg), want, "exactly enough room")


def test_reload_with_a_smaller_read_set_leaves_no_stale_tail(set31):
    p, o, g, unitigs, reads = set31
    b = p.batch(reads); b.text_mode(2); b.run()
    big = b.segments()
    assert_segments(big, expected(o, reads, 31), "the whole set")
    small = reads[100:260]
    b.reload(small)
    with pytest.raises(fa.FinitoError):   # reloaded, not run yet
        b.segments()
    b.run()
    got = b.segments()
    assert_segments(got, expected(o, small, 31), "the smaller set")
    assert len(got[0]) == len(small) + 1 and got[0][-1] == len(got[1]) < len(big[1])
    b.reload(reads); b.text_mode(0); b.run()
    assert_segments(b.segments(), big, "the whole set again")
    b.close()


def test_a_withheld_step_has_no_segments():
    """a step whose overflow list overran (tests/test_search_gpu.py::test_deque_overflow_path's recipe) has no results: FIN_ELIMIT, nothing written"""
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
            with pytest.raises(fa.FinitoError) as e:
                b.segments()
            assert e.value.code == fa.FIN_ELIMIT and "overflow list" in str(e.value) and b.device_segments_ptr() == (0, 0)
            b.close()
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0
        assert_segments(run_segments(p, reads, 2), expected(o, reads, k), "a good step afterwards")
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)
        p.close()


def test_cli_segments(tmp_path):
    rng = np.random.default_rng(98)
    g = random_genome(rng, 30000)
    unitigs = cut_unitigs(rng, g, 31, max_len=500)
    with open(tmp_path / "u.fna", "w") as f:
        for i, s in enumerate(unitigs):
            f.write(">%d\n%s\n" % (i, s))
    reads = sample_reads(rng, g, 3000, 150, err=0.01, random_frac=0.05) + [mosaic_read(rng, g, 31, 300) for _ in range(300)]
    reads = [r for r in reads if len(r) >= 31]
    with open(tmp_path / "q.fq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    run = lambda *a: subprocess.run([BIN, *a], capture_output=True, text=True)
    r = run("build-fmin", "-o", str(tmp_path / "idx"), "-u", str(tmp_path / "u.fna"), "-k", "31")
    assert r.returncode == 0, r.stderr
    o = OracleIndex.build(unitigs, 31)
    pairs = oracle_pairs(o, reads)
    nks = nks_of(reads, 31)
    want = segments_of(pairs, nks)
    read_of = np.repeat(np.arange(len(reads)), np.diff(want[0].astype(np.int64)))
    want_lines = "".join("%d\t%d\t%d\t%d\t%d\t%s\n" % (rd, s["slot"], abs(int(s["len"])), s["u"], s["off"], "-" if s["len"] < 0 else "+") for rd, s in zip(read_of, want[1]))

    def parsed(path):
        rows = np.loadtxt(path, dtype=str, delimiter="\t", ndmin=2)
        segs = np.zeros(len(rows), dtype=fa.SEGMENT_DTYPE)
        segs["slot"], segs["u"], segs["off"] = rows[:, 1].astype(np.int64), rows[:, 3].astype(np.int64), rows[:, 4].astype(np.int64)
        segs["len"] = rows[:, 2].astype(np.int64) * np.where(rows[:, 5] == "-", -1, 1)
        seg_offs = np.concatenate([[0], np.cumsum(np.bincount(rows[:, 0].astype(np.int64), minlength=len(reads)))]).astype(np.uint64)
        return seg_offs, segs

    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq"), "--gpus", "1")
    r0 = run(*common, "-o", str(tmp_path / "plain.txt"))
    assert r0.returncode == 0, r0.stderr
    r1 = run(*common, "-o", str(tmp_path / "both.txt"), "--segments", str(tmp_path / "s1.tsv"))
    assert r1.returncode == 0, r1.stderr
    assert open(tmp_path / "s1.tsv").read() == want_lines
    back, npos = fa.expand_segments(*parsed(tmp_path / "s1.tsv"), nks)
    assert np.array_equal(back.astype(np.int64), pairs)
    assert open(tmp_path / "both.txt", "rb").read() == open(tmp_path / "plain.txt", "rb").read() and os.path.getsize(tmp_path / "plain.txt") > 10 * len(reads)
    r2 = run(*common, "--segments", str(tmp_path / "s2.tsv"), "--no-text", "1")   # no -o: nothing on stdout either
    assert r2.returncode == 0 and r2.stdout == "", r2.stderr
    assert open(tmp_path / "s2.tsv").read() == want_lines
    assert np.array_equal(fa.expand_segments(*parsed(tmp_path / "s2.tsv"), nks)[0].astype(np.int64), pairs)
    found = [ln for ln in r2.stderr.splitlines() if "Total found kmers" in ln]
    assert found and found[0].split()[-1] == str(int((pairs[:, 0] != -1).sum())) and found == [ln for ln in r0.stderr.splitlines() if "Total found kmers" in ln]
    r3 = run(*common, "-o", str(tmp_path / "all.txt"), "--segments", str(tmp_path / "s3.tsv"), "--unitig-counts", str(tmp_path / "n3.tsv"), "--unitig-coverage", str(tmp_path / "c3.tsv"))
    assert r3.returncode == 0, r3.stderr
    assert open(tmp_path / "s3.tsv").read() == want_lines and open(tmp_path / "all.txt", "rb").read() == open(tmp_path / "plain.txt", "rb").read()
    counts = np.loadtxt(tmp_path / "n3.tsv", dtype=np.int64, ndmin=2)
    assert counts[:, 1].sum() == int((pairs[:, 0] != -1).sum())
    r4 = run(*common, "--segments", str(tmp_path / "s4.tsv"), "--unitig-counts", str(tmp_path / "n4.tsv"), "--no-text", "1")
    assert r4.returncode == 0 and open(tmp_path / "s4.tsv").read() == want_lines and open(tmp_path / "n4.tsv").read() == open(tmp_path / "n3.tsv").read()
