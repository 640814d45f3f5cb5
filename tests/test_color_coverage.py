"""Breadth and depth of coverage per reference, projected on the device (include/finito_amd.h: fin_colors_coverage; fin_colcov.hip).  The device
is held against the host twin (fa.unitig_color_coverage) and against the numpy model of tests/test_color_coverage_host.py (`coverage_model`, Python integers), byte
for byte; what goes into twin and model are the accumulators' own downloads -- Cover.download()'s covered[], Depth.download()'s statistics -- and nk from the
index's exported unitig ends, never a result of the call under test."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import finito_amd as fa
from tests.test_color_coverage_host import assert_coverage, coverage_model, matrix, special_colors
from tests.test_colors_host import pack, unpack, words_of
from tests.test_eqclasses import N_COLORS_OF_W, small   # noqa: F401 (the fixture: the suite's small index)
from tests.util import cut_unitigs, random_genome, rc, sample_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def nk_of(p):
    ends = p.export(fa.X_ENDS)
    return (np.diff(np.concatenate([[0], ends])) - p.k + 1).astype(np.uint64)


def expectation(col, nk, cov, dep, min_depth):
    """(twin, model) over the matrix's and the accumulators' own downloads"""
    bits = col.download()[0]
    covered = cov.download()[1] if cov is not None else None
    stats = dep.download(min_depth, want_positions=False)[1] if dep is not None else None
    return fa.unitig_color_coverage(bits, col.n_colors, nk, covered, stats, n_threads=3), coverage_model(bits, col.n_colors, nk, covered, stats)


def check(col, nk, cov, dep, min_depth, what):
    twin, want = expectation(col, nk, cov, dep, min_depth)
    got = col.coverage(cov, dep, min_depth)
    assert_coverage(twin, want, what + " (the twin)")
    assert_coverage(got, want, what)
    assert got.table.tobytes() == twin.table.tobytes() and got.uncolored == twin.uncolored
    return got


def hand_made(rng, n_unitigs, n_colors):
    """tests/test_color_coverage_host.py's matrix -- random rows, an empty row, an all-ones row, single rows for colour 0, 63, 64 and the last colour --, and a colour
    in every word: bit 63 of every full word and the last colour, together in one row and each alone"""
    bits = matrix(rng, n_unitigs, n_colors)
    every = sorted({min(64 * w + 63, n_colors - 1) for w in range(words_of(n_colors))})
    bits[0] = pack([every], n_colors)[0]
    for u, c in zip(range(1, n_unitigs - 12), every):
        bits[u] = pack([[c]], n_colors)[0]
    member = unpack(bits, n_colors)
    per_row = member.sum(axis=1)
    assert (per_row == 0).any() and (per_row == n_colors).any() and all(((per_row == 1) & (member[:, c] == 1)).any() for c in special_colors(n_colors))
    return bits


@pytest.fixture(scope="module")
def filled(small):   # noqa: F811
    """the small index with a bitmap and a depth filled by the same reads (some of them twice in the depth's eyes: the reads overlap)"""
    p, g, rng = small
    reads = sample_reads(rng, g, 200, 100, err=0.01)
    cov, dep = p.cover().add_reads(reads), p.depth().add_reads(reads)
    stats = dep.download(1, want_positions=False)[1]
    assert 0 < int((cov.download()[1] > 0).sum()) < p.n_unitigs and int(stats["max"].max()) >= 2, "the reads leave no unitig untouched, or none found twice"
    yield p, nk_of(p), cov, dep
    cov.close(); dep.close()


@pytest.mark.parametrize("chunk", [64, 0])
@pytest.mark.parametrize("W", [1, 2, 3, 64])
def test_hand_made_matrices(filled, W, chunk):
    p, nk, cov, dep = filled
    n_colors = N_COLORS_OF_W[W]
    rng = np.random.default_rng(4100 + W)
    assert p.n_unitigs >= 200 and p.n_unitigs % 64 and (chunk == 0 or p.n_unitigs > 3 * chunk)   # several chunks, the last one partial
    col = p.colors(n_colors, hand_made(rng, p.n_unitigs, n_colors))
    before = cov.download(), dep.download(2)
    p.set_option("colcov_chunk", chunk)
    try:
        for c_, d_ in ((cov, None), (None, dep), (cov, dep), (None, None)):
            for min_depth in (1, 2):
                what = "W=%d, chunk %d, cover %s, depth %s, min_depth %d" % (W, chunk, c_ is not None, d_ is not None, min_depth)
                got = check(col, nk, c_, d_, min_depth, what)
                again = col.coverage(c_, d_, min_depth)
                assert again.table.tobytes() == got.table.tobytes() and again.uncolored == got.uncolored, what + ": the second call differs"
                assert (got.covered <= got.kmers).all()
                if c_ is not None and d_ is not None:
                    assert got.covered.any() and got.depth_sum.any() and (got.depth_sum >= got.covered).all()
                    if min_depth == 1:
                        assert np.array_equal(got.solid, got.covered) and np.array_equal(got.solid_only, got.covered_only) and got.uncolored["solid"] == got.uncolored["covered"]
                    else:
                        assert (got.solid <= got.covered).all() and (got.solid < got.covered).any() and got.solid.any()
                if c_ is None:
                    assert not got.covered.any() and not got.covered_only.any() and got.uncolored["covered"] == 0
                if d_ is None:
                    assert not got.depth_sum.any() and not got.solid.any() and got.uncolored["depth_sum"] == 0
        per_row = unpack(col.download()[0], n_colors).sum(axis=1)
        assert int(got.kmers_only.sum()) + got.uncolored["kmers"] + int(nk[per_row >= 2].sum()) == int(nk.sum())
    finally:
        p.set_option("colcov_chunk", None)
    after = cov.download(), dep.download(2)
    for a, b in zip(before[0][:2] + before[1][:2], after[0][:2] + after[1][:2]):
        assert a.tobytes() == b.tobytes(), "the call changed an accumulator"
    assert before[0][2] == after[0][2] and before[1][2] == after[1][2]
    col.close()


def test_after_more_adds_and_an_upload(small):   # noqa: F811
    """accumulators of its own: the result follows every add (the scratch of an earlier call is not the answer of a later one) and a new matrix"""
    p, g, rng = small
    nk = nk_of(p)
    n_colors = 100
    rng = np.random.default_rng(4200)
    col = p.colors(n_colors, hand_made(rng, p.n_unitigs, n_colors))
    cov, dep = p.cover(), p.depth()
    p.set_option("colcov_chunk", 64)
    try:
        first = check(col, nk, cov, dep, 1, "nothing added")
        assert not first.covered.any() and not first.depth_sum.any() and first.kmers.any()
        seen = first
        for step in range(3):
            reads = sample_reads(rng, g, 60, 90, err=0.0)
            cov.add_reads(reads); dep.add_reads(reads)
            got = check(col, nk, cov, dep, 2, "after add %d" % step)
            assert (got.covered >= seen.covered).all() and int(got.depth_sum.sum()) > int(seen.depth_sum.sum())
            seen = got
        dep.reset()
        got = check(col, nk, cov, dep, 1, "the depth reset")
        assert not got.depth_sum.any() and np.array_equal(got.covered, seen.covered)
        col.upload(hand_made(rng, p.n_unitigs, n_colors))
        check(col, nk, cov, dep, 1, "a new matrix")
    finally:
        p.set_option("colcov_chunk", None)
        cov.close(); dep.close(); col.close()


def hip_runtime():
    """the HIP runtime the library itself runs on (tests/test_unitig_depth.py::device_int32's way to it)"""
    fa.lib()
    with open(os.path.join(ROOT, "finito_amd", "libfinito_amd.so"), "rb") as f:
        soname = re.search(rb"libamdhip64\.so\.[0-9]+", f.read()).group(0).decode()
    hip = C.CDLL(soname)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def test_sums_past_32_bits(small):   # noqa: F811
    """a difference array written to fin_depth_device_diff by hand: per-position depths of 2^31 - 1 over three unitigs.  Every one of them alone has a depth sum
    past 2^32; the colours' sums must match Python integers"""
    p, g, rng = small
    nk = nk_of(p)
    ends = p.export(fa.X_ENDS)
    starts = np.concatenate([[0], ends[:-1]])
    n_colors = 130
    deep = [3, 70, p.n_unitigs - 1]
    sets = [[] for _ in range(p.n_unitigs)]
    sets[deep[0]], sets[deep[1]], sets[deep[2]] = [0, 129], [129], [64, 129]
    sets[5] = [0]
    col = p.colors(n_colors, pack(sets, n_colors))
    dep = p.depth()
    D = 2 ** 31 - 1
    diff = np.zeros(p.total_len + 1, dtype=np.int32)
    for u in deep:
        diff[starts[u]] += D
        diff[ends[u]] -= D
    hip = hip_runtime()
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemcpy(C.c_void_p(dep.device_ptr()), diff.ctypes.data_as(C.c_void_p), diff.nbytes, 1) == 0   # 1 = hipMemcpyHostToDevice
    stats = dep.download(2, want_positions=False)[1]
    lens = [int(ends[u] - starts[u]) for u in deep]
    assert [int(stats["sum"][u]) for u in deep] == [n * D for n in lens] and int(stats["sum"].sum()) == sum(lens) * D and all(n * D > 2 ** 32 for n in lens)
    for chunk in (64, 0):
        p.set_option("colcov_chunk", chunk)
        try:
            got = check(col, nk, None, dep, 2, "depths of 2^31 - 1, chunk %d" % chunk)
        finally:
            p.set_option("colcov_chunk", None)
        assert int(got.depth_sum[129]) == sum(lens) * D > 2 ** 33 and int(got.depth_sum_only[129]) == lens[1] * D > 2 ** 32
        assert int(got.depth_sum[0]) == lens[0] * D and int(got.depth_sum[64]) == lens[2] * D and int(got.depth_sum_only[0]) == 0
        assert [int(got.solid[c]) for c in (0, 64, 129)] == [lens[0], lens[2], sum(lens)] and got.uncolored["depth_sum"] == 0
    dep.close(); col.close()


def raw_coverage(col, cov, dep, out, uncolored=None):
    err = C.create_string_buffer(512)
    rc_ = col.L.fin_colors_coverage(col.h, cov.h if cov is not None else None, dep.h if dep is not None else None, 1,
                                    out.ctypes.data_as(C.c_void_p) if out is not None else None, uncolored.ctypes.data_as(C.c_void_p) if uncolored is not None else None, err, 512)
    return rc_, err.value.decode()


def test_refusals(small):   # noqa: F811
    p, g, rng = small
    k = 31
    rng = np.random.default_rng(4300)
    other = fa.FinimizerIndex.build(cut_unitigs(rng, random_genome(rng, 3000), k, max_len=80), k).to_device(0)
    col = p.colors(5, matrix(rng, p.n_unitigs, 5))
    cov, dep, cov_o, dep_o = p.cover(), p.depth(), other.cover(), other.depth()
    out = np.full(6 * 8, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64).view(fa.COLOR_COVERAGE_DTYPE)
    sentinel = out.tobytes()
    try:
        for c_, d_, word in ((cov_o, None, "coverage bitmap"), (None, dep_o, "depth accumulator"), (cov_o, dep, "coverage bitmap"), (cov, dep_o, "depth accumulator")):
            rc_, msg = raw_coverage(col, c_, d_, out)
            assert rc_ == fa.FIN_EINVAL and word in msg and "different indexes or devices" in msg and out.tobytes() == sentinel
            with pytest.raises(fa.FinitoError) as e:
                col.coverage(c_, d_)
            assert e.value.code == fa.FIN_EINVAL
        rc_, msg = raw_coverage(col, cov, dep, None)
        assert rc_ == fa.FIN_EINVAL and "null" in msg
        err = C.create_string_buffer(512)
        assert col.L.fin_colors_coverage(None, cov.h, dep.h, 1, out.ctypes.data_as(C.c_void_p), None, err, 512) == fa.FIN_EINVAL and out.tobytes() == sentinel
        rc_, msg = raw_coverage(col, cov, dep, out)   # (uncolored may be NULL)
        assert rc_ == fa.FIN_OK and out[:5].tobytes() == col.coverage(cov, dep).table.tobytes() and out[5:].tobytes() == sentinel[-64:]
    finally:
        for a in (cov, dep, cov_o, dep_o, col):
            a.close()
        other.close()


def test_a_withheld_step_is_reported_until_the_reset():
    """tests/test_pileup_records.py::test_a_withheld_step_adds_nothing_and_is_reported_until_the_reset's recipe: a step whose overflow list overran is added to the
    bitmap, which flags itself; the projection then answers FIN_ELIMIT with fin_cover_download's message and writes nothing, until the reset; the same for the
    depth and for the colours"""
    k = 31
    rng = np.random.default_rng(11)
    g = random_genome(rng, 40000)
    p = fa.FinimizerIndex.build(cut_unitigs(rng, g, k, max_len=500), k).to_device(0)
    reads = sample_reads(rng, g, 500, 150)
    nk = nk_of(p)
    L = fa.lib()
    col = p.colors(3)
    windows = lambda a, b: [g[i:min(b, i + 5000 + k - 1)] for i in range(a, b, 5000)]   # (overlapping by k - 1 bases: no k-mer is lost)
    col.add_reads(windows(0, 20000), 0).add_reads(windows(10000, 40000), 2)
    cov, dep = p.cover(), p.depth()
    out = np.full(4 * 8, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64).view(fa.COLOR_COVERAGE_DTYPE)
    sentinel = out.tobytes()

    def refused(c_, d_, word):
        for _ in range(2):
            rc_, msg = raw_coverage(col, c_, d_, out[:3], out[3:])
            assert rc_ == fa.FIN_ELIMIT and "overflow list" in msg and word in msg and out.tobytes() == sentinel, (rc_, msg)
        with pytest.raises(fa.FinitoError) as e:
            col.coverage(c_, d_)
        assert e.value.code == fa.FIN_ELIMIT

    try:
        assert L.fin_set_option(b"lds_deque_limit", 1) == 0 and L.fin_set_option(b"seed_anchors", 0) == 0 and L.fin_set_option(b"debug_ovf_cap", 3) == 0
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        cov.add(b)   # nobody has looked at the step's overflow counter yet: the kernel does
        refused(cov, None, "nothing of it was set")
        refused(cov, dep, "nothing of it was set")
        got = check(col, nk, None, dep, 1, "the depth alone, the bitmap flagged")
        assert not got.depth_sum.any()
        cov.reset()
        dep.add(b)
        refused(cov, dep, "nothing of it was counted")
        dep.reset()
        got = check(col, nk, cov, dep, 1, "after the resets")
        assert not got.covered.any() and not got.depth_sum.any() and got.kmers[0] > 0 and got.kmers[2] > 0 and got.kmers[1] == 0
        col.add(b, 1)
        refused(cov, dep, "nothing of it was coloured")
        b.close()
        col.reset()
        assert L.fin_set_option(b"debug_ovf_cap", 0) == 0
        col.add_reads(windows(0, 20000), 0)
        b = p.batch(reads); b.text_mode(2); b.run(fa.FIN_MERGED)
        cov.add(b); dep.add(b)
        got = check(col, nk, cov, dep, 1, "a good step after the resets")
        assert got.covered[0] > 0 and np.array_equal(got.solid, got.covered) and got.uncolored["covered"] > 0
        b.close()
    finally:
        L.fin_set_option(b"lds_deque_limit", 16); L.fin_set_option(b"seed_anchors", 1); L.fin_set_option(b"debug_ovf_cap", 0)
        for a in (cov, dep, col):
            a.close()
        p.close()


def canonical_kmers(seqs, k):
    out = set()
    for s in seqs:
        for i in range(len(s) - k + 1):
            m = s[i:i + k]
            out.add(min(m, rc(m)))
    return out


def test_three_references_coloured_by_search():
    """tests/test_assign.py's kind of index: a shared piece and three private ones, cut into unitigs and coloured by searching every reference.  Every k-mer of a
    unitig shares its colour set, so kmers[c] is the number of distinct canonical k-mers of reference c; reads drawn from reference 0 alone cover k-mers of its own
    and none that only another reference has"""
    k = 31
    rng = np.random.default_rng(4400)
    shared, priv = random_genome(rng, 6000), [random_genome(rng, 3000) for _ in range(3)]
    unitigs = []
    for piece in [shared] + priv:
        unitigs += cut_unitigs(rng, piece, k, max_len=300)
    p = fa.FinimizerIndex.build(unitigs, k).to_device(0)
    col = p.colors(3)
    for c in range(3):
        col.add_reads([shared, priv[c]], c)
    try:
        sizes = [len(canonical_kmers([shared, priv[c]], k)) for c in range(3)]
        own = [len(canonical_kmers([priv[c]], k) - canonical_kmers([shared] + [priv[x] for x in range(3) if x != c], k)) for c in range(3)]
        assert len(canonical_kmers(unitigs, k)) == sum(len(u) - k + 1 for u in unitigs), "a k-mer in two unitigs: the sizes below would not be the sums of nk"
        bare = col.coverage()
        assert [int(x) for x in bare.kmers] == sizes and [int(x) for x in bare.kmers_only] == own and bare.uncolored["kmers"] == 0
        assert not bare.covered.any() and np.isnan(bare.mean_depth).all() and (bare.breadth == 0).all()
        reads = sample_reads(rng, shared + priv[0], 400, 100, err=0.0, random_frac=0.0)
        got = p.color_coverage(reads, col, min_depth=2)
        cov, dep = p.cover().add_reads(reads), p.depth().add_reads(reads)
        twin, want = expectation(col, nk_of(p), cov, dep, 2)
        assert_coverage(got, want, "FinimizerIndex.color_coverage")
        assert_coverage(twin, want, "the twin")
        cov.close(); dep.close()
        assert [int(x) for x in got.kmers] == sizes
        assert got.breadth_only[0] > 0 and got.covered_only[1] == 0 and got.covered_only[2] == 0 and np.array_equal(got.breadth_only[1:], [0.0, 0.0])
        assert got.covered[1] == got.covered[2] > 0 and got.covered[0] == got.covered[1] + got.covered_only[0]   # (the shared piece, and what reference 0 adds)
        found = canonical_kmers(reads, k)
        assert int(got.covered[0]) == len(found & canonical_kmers([shared, priv[0]], k)) and 0 < got.breadth[0] <= 1 and got.mean_depth[0] >= 1
        assert 0 < int(got.solid[0]) < int(got.covered[0])
    finally:
        col.close(); p.close()
