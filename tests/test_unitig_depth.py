"""The per-position depth accumulated on the device (include/finito_amd.h: fin_depth, fin_batch_add_depth, fin_search_batch_unitig_depth; fin_depth.hip).

The expected depth is always np.bincount over the ORACLE's found pairs of the same reads (oracle/: the reference's algorithm restated on the CPU), mapped through
the oracle's unitig ends to text positions, never this library's own pairs; every comparison is exact equality of the whole array and of every unitig's three
numbers (sum, max, n_at_least), and total == depth.sum()."""
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


def device_int32(ptr, n):
    """n int32 words of device memory (for Depth.device_ptr(): the difference array in HBM), copied by the very HIP runtime the library runs on: it is opened
    by the soname the library itself was linked against, which the loader answers with the copy that is already in the process -- another copy of the runtime
    (a second installation, one bundled with a Python package) would know nothing of this process's device memory"""
    import ctypes as C
    import re
    fa.lib()
    with open(os.path.join(ROOT, "finito_amd", "libfinito_amd.so"), "rb") as f:
        soname = re.search(rb"libamdhip64\.so\.[0-9]+", f.read()).group(0).decode()
    hip = C.CDLL(soname)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(n, dtype=np.int32)
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), 4 * n, 2) == 0   # 2 = hipMemcpyDeviceToHost
    return out


class Want:
    """depth (uint32 per text position) and, per unitig, sum / max / the positions with depth >= min_depth; found = the found pairs"""

    def __init__(self, pairs, ends, depth=None):
        self.ends = np.asarray(ends, dtype=np.int64)
        self.starts = np.concatenate([[0], self.ends[:-1]])
        if depth is None:
            p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
            p = p[p[:, 0] >= 0]
            depth = np.bincount(self.starts[p[:, 0]] + p[:, 1], minlength=int(self.ends[-1]))
        self.depth = np.asarray(depth, dtype=np.int64)
        assert len(self.depth) == int(self.ends[-1]) and self.depth.max(initial=0) < 2 ** 32
        self.found = int(self.depth.sum())

    def stats(self, min_depth=1):
        s = np.zeros(len(self.ends), dtype=fa.DEPTH_STAT_DTYPE)
        s["sum"] = np.add.reduceat(self.depth, self.starts)
        s["max"] = np.maximum.reduceat(self.depth, self.starts)
        s["n_at_least"] = np.add.reduceat((self.depth >= min_depth).astype(np.int64), self.starts)
        return s

    def __add__(self, other):
        return Want(None, self.ends, self.depth + other.depth)

    def times(self, n):
        return Want(None, self.ends, n * self.depth)


def oracle_pairs(o, reads, strands=fa.FIN_MERGED):
    if strands == fa.FIN_MERGED:
        return o.search_batch(reads, n_threads=8)[0]
    return np.array([x for r in reads for x in o.search(r)[0]], dtype=np.int64).reshape(-1, 2)   # FinimizerIndex::search on each read


def expected(o, reads, strands=fa.FIN_MERGED):
    return Want(oracle_pairs(o, reads, strands), o.ends())


def assert_stats(stats, want, min_depth, what=""):
    ws = want.stats(min_depth)
    assert stats.dtype == fa.DEPTH_STAT_DTYPE and stats.shape == ws.shape, what
    for name in ("sum", "max", "n_at_least"):
        bad = np.nonzero(stats[name] != ws[name])[0]
        assert len(bad) == 0, "%s: %s differs in %d unitigs, first %d: got %d, oracle %d" % (what, name, len(bad), bad[0], stats[name][bad[0]], ws[name][bad[0]])


def assert_depth(got, want, what="", min_depth=1):
    depth, stats, total = got
    assert depth.dtype == np.uint32 and depth.shape == want.depth.shape, what
    bad = np.nonzero(depth.astype(np.int64) != want.depth)[0]
    assert len(bad) == 0, "%s: %d positions differ, first %d: got %d, oracle %d" % (what, len(bad), bad[0], depth[bad[0]], want.depth[bad[0]])
    assert_stats(stats, want, min_depth, what)
    assert total == want.found == int(depth.astype(np.int64).sum()), what


def assert_inputs_show_something(want):
    """conditions on the inputs, checked on the oracle's expectation: some position has depth >= 3, some has depth 0, some unitig has two different nonzero depths"""
    assert (want.depth >= 3).any() and (want.depth == 0).any()
    two = False
    for a, b in zip(want.starts, want.ends):
        d = np.unique(want.depth[a:b]); two = two or len(d[d > 0]) >= 2
    assert two


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
def test_depth_of_every_read_family_in_every_text_mode(k):
    """text modes 0, 1 and 2: in mode 2 the depth of the fast path's reads comes from their records; k = 127 leaves no records, every read goes through the pair
    scan.  The add changes neither records nor pairs: text and pairs afterwards are the oracle's.  No depth in the last k - 1 positions of any unitig"""
    rng = np.random.default_rng(100 + k)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=max(700, 4 * k))
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    assert np.array_equal(p.export(fa.X_ENDS), o.ends())
    reads = read_families(rng, g, k, unitigs)
    e1 = oracle_pairs(o, reads)
    want = Want(e1, o.ends())
    assert_inputs_show_something(want)
    full = [r for r in reads if len(r) >= k]   # (the text formatter wants a k-mer in every read)
    e2 = oracle_pairs(o, full)
    want_full = Want(e2, o.ends())
    want_text, at = [], 0
    for r in full:
        want_text.append(format_pairs(e2[at:at + len(r) - k + 1])); at += len(r) - k + 1
    want_text = "".join(want_text).encode()
    tail = np.zeros(len(want.depth), dtype=bool)   # the last k - 1 positions of every unitig
    for e in o.ends():
        tail[e - (k - 1):e] = True
    d = p.depth()
    assert d.device_ptr()
    for mode in (0, 1, 2):
        b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        got = d.reset().add(b).download()
        assert_depth(got, want, "k=%d text mode %d" % (k, mode))
        assert not got[0][tail].any()
        info = b.run_info()
        if mode == 2 and info["fast_path"]:
            with pytest.raises(fa.FinitoError):
                b.download()
        else:
            pairs, npos = b.download()
            assert npos == want.found and np.array_equal(pairs.astype(np.int64), e1)
        b.reload(full); b.run(fa.FIN_MERGED)
        assert_depth(d.reset().add(b).download(), want_full, "k=%d text mode %d, reads with k-mers" % (k, mode))
        assert b.text() == want_text, "text after add, k=%d mode %d" % (k, mode)
        assert b.download(want_pairs=False)[1] == want_full.found
        b.close()
    # an empty batch, a batch of reads without k-mers, a batch of 300 absent reads and an all-N read
    for rd in ([], ["", "AC"], [random_genome(rng, 200) for _ in range(300)] + ["N" * 200]):
        b = p.batch(rd); b.text_mode(2); b.run(fa.FIN_MERGED)
        assert_depth(d.reset().add(b).download(), expected(o, rd) if rd else Want(np.zeros((0, 2)), o.ends()), "k=%d %d reads" % (k, len(rd)))
        b.close()
    d.close(); p.close()


def test_the_three_accumulators_agree(set31):
    """from the same run: (depth > 0) is the bitmap, a unitig's summed depth is its hit count, n_at_least at 1 is `covered`; n_at_least at other thresholds"""
    p, o, g, unitigs, reads = set31
    want = expected(o, reads)
    for mode in (2, 0):
        b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
        h, c, d = p.hits(), p.cover(), p.depth()
        h.add(b); d.add(b); c.add(b)
        depth, stats, total = d.download(min_depth=1)
        assert_depth((depth, stats, total), want, "depth beside hits and cover, mode %d" % mode)
        bits, covered, n_covered = c.download()
        counts, n_hits = h.download()
        flat = np.zeros(64 * len(bits), dtype=np.uint8)
        flat[:len(depth)] = depth > 0
        assert np.array_equal(np.packbits(flat, bitorder="little").view(np.uint64), bits)
        assert np.array_equal(stats["sum"], counts) and total == n_hits
        assert np.array_equal(stats["n_at_least"].astype(np.uint64), covered) and int(stats["n_at_least"].sum()) == n_covered
        assert np.array_equal(counts, profile_of(oracle_pairs(o, reads), p.n_unitigs))
        for t in (2, 5, 2 ** 32 - 1):
            positions, st, tot = d.download(min_depth=t, want_positions=False)
            assert positions is None and tot == want.found
            assert_stats(st, want, t, "min_depth %d, mode %d" % (t, mode))
        assert want.stats(2)["n_at_least"].sum() > want.stats(5)["n_at_least"].sum() > 0 and not want.stats(2 ** 32 - 1)["n_at_least"].any()
        h.close(); c.close(); d.close(); b.close()


def test_non_disjoint_sets():
    """identical unitigs, near-duplicates, reverse-complement copies (tests/util.py::defer_family_case): only the copy the reference reports counts"""
    rng = np.random.default_rng(555)
    for case in range(10):
        k = (31, 16, 21, 47, 63)[case % 5]
        g, unitigs, reads = defer_family_case(rng, case, k)
        p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
        o = OracleIndex.build(unitigs, k)
        want = expected(o, reads)
        assert want.found > 0
        for mode in (2, 0):
            b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
            d = p.depth()
            assert_depth(d.add(b).download(), want, "case %d k=%d mode %d" % (case, k, mode))
            d.close(); b.close()
        p.close()


@pytest.mark.parametrize("opts", [{"kernel": 4}, {"kernel": 3}, {"kernel": 2}, {"kernel": 0}, {"fast_path": 0}, {"pp_park": 0}],
                         ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
@pytest.mark.parametrize("strands", [fa.FIN_MERGED, fa.FIN_FWD], ids=["merged", "fwd"])
def test_kernels_strands_and_options(set31, opts, strands):
    p, o, g, unitigs, reads = set31
    rd = reads if strands == fa.FIN_MERGED else reads[:400]
    want = expected(o, rd, strands)
    assert want.found > 0
    for name, v in opts.items():
        p.set_option(name, v)
    try:
        for mode in (2, 0):
            b = p.batch(rd); b.text_mode(mode); b.run(strands)
            d = p.depth()
            assert_depth(d.add(b).download(), want, "%s mode %d" % (opts, mode))
            assert_depth(d.add(b).download(), want.times(2), "%s mode %d, the same run twice" % (opts, mode))
            d.close(); b.close()
    finally:
        for name in opts:
            p.set_option(name, None)


@pytest.mark.parametrize("tile", [0, 64, 257], ids=lambda t: "tile=%d" % t)
def test_accumulation_downloads_in_between_reset_and_the_scan_in_small_tiles(set31, tile):
    """three read sets into one accumulator give the sum, a download in between does not disturb it, a second accumulator stays untouched, reset gives zeros.
    debug_depth_tile = 64 / 257: the 40 000-base text is 625 / 156 tiles in 10 / 3 chunks of the second level (64 tiles each), the last tile and chunk partial"""
    p, o, g, unitigs, reads = set31
    assert p.total_len > 2 * 64 * 257
    sets = [reads[:500], reads[500:1100], reads[1100:] + reads[:37]]
    wants = [expected(o, s) for s in sets]
    p.set_option("debug_depth_tile", tile)
    try:
        d, d2 = p.depth(), p.depth()
        assert d.device_ptr() and d.device_ptr() != d2.device_ptr()
        b = p.batch(sets[0]); b.text_mode(2)
        for i, s in enumerate(sets):
            if i:
                b.reload(s)
            b.run(fa.FIN_MERGED)
            d.add(b)                              # behind the run, on its stream, no wait in between
            if i == 1:
                d2.add(b)
                assert_depth(d2.download(), wants[1], "second accumulator")
                assert_depth(d.download(min_depth=2), wants[0] + wants[1], "a download in between", min_depth=2)
        total = wants[0] + wants[1] + wants[2]
        assert_depth(d.download(), total, "three read sets in one accumulator")
        assert_depth(d.download(min_depth=3), total, "downloaded again", min_depth=3)
        assert_depth(d2.download(), wants[1], "second accumulator untouched")
        d.add(b)
        assert_depth(d.download(), total + wants[2], "the last run twice")
        depth, stats, tot = d.reset().download()
        assert tot == 0 and not depth.any() and not stats["sum"].any() and not stats["max"].any() and not stats["n_at_least"].any()
        assert_depth(d.add(b).download(), wants[2], "after reset")
        b.close(); d.close(); d2.close()
    finally:
        p.set_option("debug_depth_tile", None)


@pytest.mark.parametrize("n_unitigs", [1, 3])
def test_contention_few_unitigs(n_unitigs):
    """200 000 reads on 30 000 bases: every entry of the difference array is contended; one unitig of 30 000 bases for the statistics"""
    g = synth.genome(30000, seed=7 + n_unitigs)
    gs = g.tobytes().decode()
    cuts = [0, len(gs)] if n_unitigs == 1 else [0, 9000, 21000, len(gs)]
    unitigs = [gs[max(0, a - 30) if a else 0:b] for a, b in zip(cuts[:-1], cuts[1:])]   # (overlapping by k - 1: every k-mer in one unitig)
    rd = synth.reads(g, 200_000, seed=11)
    p = fa.FinimizerIndex.build(unitigs, 31).to_device(0)
    assert p.n_unitigs == n_unitigs
    o = OracleIndex.build(unitigs, 31)
    want = expected(o, rd.as_tuple())
    assert want.found > 10_000_000 and want.depth.max() > 500
    for mode in (2, 0):
        b = p.batch(rd.as_tuple()); b.text_mode(mode); b.run(fa.FIN_MERGED)
        d = p.depth()
        assert_depth(d.add(b).download(min_depth=400), want, "%d unitigs, mode %d" % (n_unitigs, mode), min_depth=400)
        d.close(); b.close()
    stats, npos = p.unitig_depth(rd.as_tuple(), min_depth=400)
    assert_stats(stats, want, 400, "unitig_depth") ; assert npos == want.found
    p.close()


def test_many_unitigs():
    """more than 5e4 unitigs of at most 40 bases at k = 21: several unitigs share a tile and a lane of the statistics kernel, and the -1 of one unitig sits next
    to the +1 of the next"""
    g = synth.genome(1_000_000, seed=5)
    u = synth.unitigs(g, 21, max_len=40)
    rd = synth.reads(g, 100_000, seed=6)
    p = fa.FinimizerIndex.build(u.as_tuple(), 21).to_device(0)
    assert p.n_unitigs >= 50_000
    o = OracleIndex.build(u.as_tuple(), 21)
    assert int(np.diff(np.concatenate([[0], o.ends()])).max()) <= 40
    want = expected(o, rd.as_tuple())
    assert (want.stats()["sum"] > 0).sum() > 40_000 and want.depth.max() >= 3
    for mode in (2, 0):
        b = p.batch(rd.as_tuple()); b.text_mode(mode); b.run(fa.FIN_MERGED)
        d = p.depth()
        assert_depth(d.add(b).download(min_depth=2), want, "%d unitigs, mode %d" % (p.n_unitigs, mode), min_depth=2)
        d.close(); b.close()
    p.close()


def test_depth_from_host_buffers_in_many_sub_batches(set31):
    p, o, g, unitigs, reads = set31
    want = expected(o, reads)
    one, npos1 = p.unitig_depth(reads)
    assert_stats(one, want, 1, "one call"); assert npos1 == want.found
    for sub, depth in ((3000, 3), (20000, 1), (500, 8)):
        p.set_option("pipeline_kmers", sub); p.set_option("pipeline_depth", depth)
        try:
            many, npos = p.unitig_depth(reads, min_depth=2)
            d = p.depth()
            got = d.add_reads(reads).download()
            d.close()
        finally:
            p.set_option("pipeline_kmers", None); p.set_option("pipeline_depth", None)
        assert_stats(many, want, 2, "sub-batches of %d k-mers" % sub); assert npos == want.found
        assert_depth(got, want, "add_reads in sub-batches of %d k-mers" % sub)
    fwd, nf = p.unitig_depth(reads[:300], fa.FIN_FWD)
    wf = expected(o, reads[:300], fa.FIN_FWD)
    assert_stats(fwd, wf, 1, "forward only"); assert nf == wf.found
    for rd in ([], ["", "ACG"]):
        st, n = p.unitig_depth(rd)
        assert n == 0 and st.shape == (p.n_unitigs,) and not st["sum"].any() and not st["max"].any() and not st["n_at_least"].any()
    # chunks streamed into one resident accumulator, downloaded once
    d = p.depth()
    d.add_reads(reads[:700]).add_reads(reads[700:]).add_reads([])
    assert_depth(d.download(), want, "add_reads in two chunks")
    # the host-side depth over records + stream is the device's
    recs, stream = p.search_reads_records(reads)
    assert np.array_equal(fa.records_depth(recs, stream, 31, p.export(fa.X_ENDS)), d.download()[0])
    assert np.array_equal(fa.records_depth(recs, stream, 31, o.ends()).astype(np.int64), want.depth)
    d.close()


class _Borrowed:
    """an accumulator handle presented together with an index it does not belong to"""

    def __init__(self, index, depth):
        self.index, self.h, self.L = index, depth.h, depth.L


def test_wrong_pairing_is_refused_and_the_device_stays_usable(set31):
    p, o, g, unitigs, reads = set31
    rng = np.random.default_rng(3)
    other = fa.FinimizerIndex.build(cut_unitigs(rng, random_genome(rng, 5000), 31, max_len=300), 31).to_device(0)
    d, d_other = p.depth(), other.depth()
    b = p.batch(reads[:200])
    with pytest.raises(fa.FinitoError) as e:   # a batch that has not run
        d.add(b)
    assert e.value.code == fa.FIN_EINVAL and "not run" in str(e.value)
    b.text_mode(2); b.run(fa.FIN_MERGED)
    with pytest.raises(fa.FinitoError) as e:   # the accumulator of another index
        d_other.add(b)
    assert e.value.code == fa.FIN_EINVAL and "different" in str(e.value)
    with pytest.raises(fa.FinitoError) as e:   # ... through the host-buffer loop too
        fa.Depth.add_reads(_Borrowed(p, d_other), reads[:10])
    assert e.value.code == fa.FIN_EINVAL and "another index" in str(e.value)
    with pytest.raises(fa.FinitoError):        # no replica on that device
        p.depth(device=63)
    assert not d_other.download()[0].any()
    assert_depth(d.add(b).download(), expected(o, reads[:200]), "after the refusals")
    b.close(); d.close(); d_other.close(); other.close()


def test_a_withheld_step_adds_nothing_and_is_reported_until_the_reset():
    """a step whose overflow list overran (tests/test_unitig_coverage.py::test_a_withheld_step_sets_nothing_and_is_reported_until_the_reset's recipe) has no
    results: the add reads the counter itself, adds nothing and flags the accumulator; fin_depth_download reports FIN_ELIMIT until the reset, after which the
    accumulator is clean and usable"""
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    unitigs = cut_unitigs(rng, g, k, max_len=500)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    o = OracleIndex.build(unitigs, k)
    reads = sample_reads(rng, g, 500, 150)
    want = expected(o, reads)
    L = fa.lib()
    d = p.depth()
    try:
        assert L.fin_set_option(b"lds_deque_limit", 1) == 0 and L.fin_set_option(b"seed_anchors", 0) == 0 and L.fin_set_option(b"debug_ovf_cap", 3) == 0
        for mode in (0, 2):
            b = p.batch(reads); b.text_mode(mode); b.run(fa.FIN_MERGED)
            d.add(b)                                   # nobody has looked at the step's overflow counter yet: the kernel does
            with pytest.raises(fa.FinitoError) as e:
                d.download()
            assert e.value.code == fa.FIN_ELIMIT and "overflow list" in str(e.value)
            with pytest.raises(fa.FinitoError) as e:   # ... and keeps saying so
                d.download()
            assert e.value.code == fa.FIN_ELIMIT
            depth, stats, total = d.reset().download()
            assert total == 0 and not depth.any() and not stats["sum"].any(), "a withheld step added something (mode %d)" % mode
            with pytest.raises(fa.FinitoError) as e:   # once the host knows (a download looked), the add itself refuses
                b.download(want_pairs=False) if mode == 0 else b.text()
            assert e.value.code == fa.FIN_ELIMIT
            with pytest.raises(fa.FinitoError) as e:
                d.add(b)
            assert e.value.code == fa.FIN_ELIMIT
            b.close()
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        assert_depth(d.add(b).download(), want, "a good step after the reset")
        b.close()
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)
        d.close(); p.close()


def test_hand_made_pairs_and_places_outside_the_index(set31):
    """hand-made pairs (fin_batch_set_pairs; the flat scan): an ascending run of 200, a descending run of 150 that ends at a unitig's last k-mer,
    10,11,12,11,10,9,10, then 5,5,5 (depth 3), a single slot, a whole unitig descending -- and a unitig number the index does not have, the first position beyond the
    text, one of them directly behind a good ascending run that it would continue: skipped, everything else counted, FIN_EINVAL until the reset"""
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
    for offs in (range(0, 200), range(L_ - 1, L_ - 1 - 150, -1), [10, 11, 12, 11, 10, 9, 10], [5, 5, 5], [260], range(250, 260)):
        for x in offs:
            good[at] = (u_long, x); at += 1
        at += 1 + int(rng.integers(0, 3))
    u2 = (u_long + 1) % len(ends)
    for x in range(int(lens[u2]) - 31, -1, -1):   # a whole unitig, descending
        good[at] = (u2, x); at += 1
    assert at < n - 40
    want = Want(good, ends)
    s = int(want.starts[u_long])
    assert want.depth[s + 5] == 4 and want.depth[s + 10] == 4 and want.depth[s + 11] == 3 and want.depth[s + 9] == 2 and want.depth[s + 260] == 1
    d = p.depth()
    b.set_pairs(good)
    assert_depth(d.reset().add(b).download(), want, "hand-made runs")
    assert_depth(d.add(b).download(), want.times(2), "hand-made runs twice")
    last = p.n_unitigs - 1
    bad = good.copy()
    bad[at + 2] = (p.n_unitigs + 5, 0)                                   # a unitig the index does not have
    bad[at + 4] = (last, int(lens[-1]))                                  # the first position beyond the text
    bad[at + 6] = (last, int(lens[-1]) + 100000)
    bad[at + 8] = (-7, 3)                                                # a negative unitig number that is not "absent"
    # a good ascending run up to the text's very last position (a place of the index, if of no k-mer), and the slot behind it that would continue it
    run = 20
    for i in range(run):
        bad[at + 12 + i] = (last, int(lens[-1]) - run + i)
    bad[at + 12 + run] = (last, int(lens[-1]))
    inside = bad.copy()
    for i in (2, 4, 6, 8, 12 + run):
        inside[at + i] = (-1, -1)
    want_bad = Want(inside, ends)
    assert want_bad.depth[-1] == 1 and want_bad.found == want.found + run
    b.set_pairs(bad)
    d.reset().add(b)
    with pytest.raises(fa.FinitoError) as e:
        d.download()
    assert e.value.code == fa.FIN_EINVAL and "outside the index" in str(e.value)
    with pytest.raises(fa.FinitoError) as e:   # ... until the reset
        d.download(want_positions=False)
    assert e.value.code == fa.FIN_EINVAL
    # everything else was counted and no bad slot left half a range: the difference array itself, read through the device pointer, sums to the expectation
    diff = device_int32(d.device_ptr(), p.total_len + 1)
    assert np.array_equal(np.cumsum(diff[:-1].astype(np.int64)), want_bad.depth) and int(diff.astype(np.int64).sum()) == 0 and diff[-1] == -1
    b.set_pairs(good)
    assert_depth(d.reset().add(b).download(), want, "after the reset")
    b.set_pairs(inside)
    assert_depth(d.reset().add(b).download(), want_bad, "the run up to the text's last position")
    d.close(); b.close()


def test_cli_unitig_depth(tmp_path):
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
    lines = lambda t: "".join("%d\t%d\t%d\t%d\t%d\n" % (u, lens[u] - 31 + 1, s["sum"], s["max"], s["n_at_least"]) for u, s in enumerate(want.stats(t)))
    covered = want.stats(1)["n_at_least"]
    want_cover = "".join("%d\t%d\t%d\n" % (u, lens[u] - 31 + 1, int(c)) for u, c in enumerate(covered))
    want_counts = "".join("%d\t%d\n" % (u, int(c)) for u, c in enumerate(profile_of(pairs, len(unitigs))))
    assert lines(1) != lines(3) and want.depth.max() >= 3
    common = ("search-fmin", "-i", str(tmp_path / "idx"), "-q", str(tmp_path / "q.fq"), "--gpus", "1")
    r0 = run(*common, "-o", str(tmp_path / "plain.txt"))
    assert r0.returncode == 0, r0.stderr
    r1 = run(*common, "-o", str(tmp_path / "both.txt"), "--unitig-depth", str(tmp_path / "d1.tsv"))   # --min-depth defaults to 1
    assert r1.returncode == 0, r1.stderr
    assert open(tmp_path / "d1.tsv").read() == lines(1)
    assert open(tmp_path / "both.txt", "rb").read() == open(tmp_path / "plain.txt", "rb").read() and os.path.getsize(tmp_path / "plain.txt") > 10 * len(reads)
    r2 = run(*common, "-o", str(tmp_path / "all.txt"), "--unitig-depth", str(tmp_path / "d2.tsv"), "--min-depth", "3", "--unitig-coverage", str(tmp_path / "c2.tsv"),
             "--unitig-counts", str(tmp_path / "n2.tsv"))
    assert r2.returncode == 0, r2.stderr
    assert open(tmp_path / "d2.tsv").read() == lines(3) and open(tmp_path / "c2.tsv").read() == want_cover and open(tmp_path / "n2.tsv").read() == want_counts
    assert open(tmp_path / "all.txt", "rb").read() == open(tmp_path / "plain.txt", "rb").read()
    r3 = run(*common, "--unitig-depth", str(tmp_path / "d3.tsv"), "--min-depth", "1", "--no-text", "1")   # no -o: nothing on stdout either
    assert r3.returncode == 0 and r3.stdout == "" and open(tmp_path / "d3.tsv").read() == lines(1)
    found = [ln for ln in r3.stderr.splitlines() if "Total found kmers" in ln]
    assert found and found[0].split()[-1] == str(want.found) and found == [ln for ln in r0.stderr.splitlines() if "Total found kmers" in ln]
